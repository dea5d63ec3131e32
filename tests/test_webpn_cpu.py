"""The host parse and arithmetic of the decoder for the first frame of animated WebP files (ke_webpn_parse.h and, through it, the
three still decoders' headers) built for the CPU and held against Pillow, bit for bit.  The rule: a taken file is one Pillow
opens, and ``np.asarray(Image.open(f))`` is equal in shape, mode and every byte.  Every valid case of tests/_webpn_cases.py has to
be taken; the invalid ones carry the status their rule names; damaged files are refused or decoded as Pillow decodes them.  No
GPU needed: the headers are compiled with the host C++ compiler (tests/_webpn_cpu.cpp) into a program of its own, under
AddressSanitizer and UBSan, which reads the case files from a temporary directory; the probes of the built library are host
code."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _webp_cases as W  # noqa: E402
import _webpa_cases as A  # noqa: E402
import _webpl_cases as L  # noqa: E402
import _webpn_cases as N  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The sanitised program"""
    out = str(tmp_path_factory.mktemp("webpn_san") / "webpn_san")
    base = [_cxx(), "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DKE_WEBPN_MAIN", "-I", CSRC,
            os.path.join(ROOT, "tests", "_webpn_cpu.cpp"), "-o", out]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    return out


def run(exe, work, files) -> list:
    """[(status, pixels or None, (width, height, channels, meta, codec, frames))] of ``files`` (bytes) through the program"""
    work = str(work)
    for k, data in enumerate(files):
        with open(os.path.join(work, f"{k}.webp"), "wb") as f:
            f.write(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    done = subprocess.run([exe, work, str(len(files))], env=env, capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-500:] + done.stderr[-4000:]
    lines = done.stdout.split("\n")[:-1]
    assert len(lines) == len(files)
    out = []
    for k, line in enumerate(lines):
        st, w, h, ch, *rest = (int(v) for v in line.split())
        px = np.fromfile(os.path.join(work, f"{k}.out"), np.uint8).reshape(h, w, ch) if st == N.OK else None
        out.append((st, px, (w, h, ch, *rest)))
    return out


@pytest.fixture(scope="module")
def valid(exe, tmp_path_factory):
    """The valid cases through the program, once: [((family, name, bytes), (status, pixels, info))]"""
    cases = N.valid_cases()
    return list(zip(cases, run(exe, tmp_path_factory.mktemp("webpn_valid"), [d for _, _, d in cases])))


def test_census():
    """Every family is present, each codec is frame 0 with three and with four channels, and the sizes the issue names occur."""
    count = N.census()
    print("valid files:", dict(count))
    assert all(count[f] > 0 for f in N.FAMILIES) and all(count[c] >= 40 for c in N.CODECS) and min(count["rgb"], count["rgba"]) >= 100
    names = {name for _, name, _ in N.valid_cases()}
    for codec in N.CODECS:
        for alpha in (0, 1):
            assert {f"{codec}_{p}_alpha{alpha}" for p in ("nw", "ne", "sw", "se", "centre")} <= names
            assert {f"{codec}_{t}_alpha{alpha}" for t in ("1x1_on_1x1", "1x1_at_2_2_of_3x3", "1_wide", "1_high")} <= names
        assert {f"{codec}_bits{b}" for b in range(4)} <= names and f"{codec}_12_frames" in names and f"{codec}_inside" in names
    for cw in list(range(1, 10)) + [15, 16, 17]:
        assert any(n.startswith(f"w{cw}_alpha0_") for n in names) and any(n.startswith(f"w{cw}_alpha1_") for n in names)
    assert sum("garbage" in n for n in names) >= 6


def test_every_valid_case_is_taken_and_equals_pillow(valid):
    """Shape (so the mode: RGBA with the VP8X alpha flag, RGB without), and every byte; the caveats; outside the frame zeros."""
    for (family, name, data), (st, px, info) in valid:
        ref = N.pillow_pixels(data)
        assert ref is not None, (family, name)
        assert st == N.OK, (family, name, st)
        assert px.shape == ref.shape and ref.shape[2] == (4 if data[20] & N.ALPHA else 3), (family, name, px.shape, ref.shape)
        assert np.array_equal(px, ref), (family, name)
        assert info[3] == int(N.with_meta(data)), (family, name)
    placed = {name: px for (family, name, _), (_, px, _) in valid if family == "placed"}
    corner = placed["lossy_se_alpha1"]
    assert not corner[:12].any() and not corner[:, :12].any() and corner[12:, 12:, 3].all()


def test_frame_pixels_are_the_still_decoders(valid):
    """The frame rectangle holds what Pillow gives for the same sub-chunks wrapped as a still file (alpha 255 where the frame has
    none, dropped where the canvas is RGB) -- checked on Pillow's side, which is what lets the still decoders' kernels serve."""
    rng = np.random.default_rng(5)
    for codec in N.CODECS:
        f = N._frame(rng, codec, 38, 22, 1)
        for alpha in (False, True):
            canvas = N.pillow_pixels(N.simple(f, (48, 32), 4, 6, alpha))
            still = N.pillow_pixels(f.still(alpha))
            if still.shape[2] == 3:
                still = np.dstack([still, np.full(still.shape[:2], 255, np.uint8)])
            inside = canvas[6:28, 4:42]
            assert np.array_equal(inside, still[..., :canvas.shape[2]]), (codec, alpha)
            outside = canvas.copy()
            outside[6:28, 4:42] = 0
            assert not outside.any(), (codec, alpha)


def test_invalid_cases_carry_the_status_their_rule_names(exe, tmp_path):
    cases = N.invalid_cases()
    got = run(exe, tmp_path, [d for _, d, _ in cases])
    for (name, data, expected), (st, _, _) in zip(cases, got):
        assert st == expected, (name, st)
        if expected == N.CORRUPT:
            assert N.pillow_pixels(data) is None, name                 # Pillow fails too
    assert len(cases) >= 30 and sum(e == N.CORRUPT for _, _, e in cases) >= 20


def test_refusals_pillow_does_not_share_are_listed_by_name(exe, tmp_path):
    """Status 1 although Pillow opens the file: each with its reason in _webpn_cases.UNSHARED_REFUSALS"""
    cases = N.unshared_cases()
    got = run(exe, tmp_path, [d for _, d in cases])
    for (name, data), (st, _, _) in zip(cases, got):
        assert name in N.UNSHARED_REFUSALS and st == N.UNSUPPORTED, (name, st)
        assert N.pillow_pixels(data) is not None, name
    assert set(N.UNSHARED_REFUSALS) - {n for n, _ in cases} == {"frame_0_over_the_lossy_cap"}


def test_damage(exe, tmp_path):
    """Every valid file cut at half its length, before its last byte and at byte 30 (Pillow opens none of those: it wants the
    whole RIFF), and 2 000 single-byte changes behind the RIFF header: status 0 => Pillow opens the file to the same pixels.  Not
    vacuous: Pillow still opens at least a quarter of the damaged files (the first run: 1 289 of 2 936, 44 %), and of those the decoder
    has to take three quarters, the rule of test_gpu_webpa.py (the first run of this CPU build: 1 123 of 1 289, 87 %; what is
    left out are files Pillow still opens and this decoder leaves alone on purpose -- an ANMF header whose size is no longer its
    bitstream's, the refusals of _webpn_cases.UNSHARED_REFUSALS -- or as something it does not claim to reproduce)."""
    damaged = N.cut_cases() + N.byte_changes(2000)
    got = run(exe, tmp_path, [d for _, d in damaged])
    pillow_ok = taken = 0
    for (name, data), (st, px, _) in zip(damaged, got):
        assert st in (N.OK, N.UNSUPPORTED, N.CORRUPT), name
        ref = N.pillow_pixels(data)
        pillow_ok += ref is not None
        if st == N.OK:
            taken += 1
            assert ref is not None, f"{name}: taken where Pillow refuses"
            assert px.shape == ref.shape and np.array_equal(px, ref), f"{name}: taken where Pillow differs"
    print(f"damage: {len(damaged)} files, Pillow opens {pillow_ok}, the decoder takes {taken}")
    assert len(damaged) >= 2000 + 3 * len(N.valid_cases()) and 4 * pillow_ok >= len(damaged) and 4 * taken >= 3 * pillow_ok


# ---- the built library's host-only probes ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def K():
    if not os.path.exists(os.path.join(ROOT, "kobato-eyes_amd", "libkeyes_hip.so")):
        subprocess.check_call(["bash", os.path.join(ROOT, "kobato-eyes_amd", "build.sh")])
    import kobato_eyes_amd

    return kobato_eyes_amd


def _probe(lib, kind: str, files: list):
    n = len(files)
    flat = np.frombuffer(b"".join(files) + b"\0", np.uint8)
    sizes = np.array([len(f) for f in files], np.uint64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    w, h, c, st = (np.zeros(n, np.int32) for _ in range(4))
    ptr = lambda a: C.c_void_p(a.ctypes.data)                          # noqa: E731
    fn = getattr(lib, f"ke_{kind}_probe")
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn(ptr(flat), ptr(offsets), ptr(sizes), n, ptr(w), ptr(h), ptr(c), ptr(st)) == 0
    return w, h, c, st


def _all_webp_files() -> list:
    """Every valid, refused and damaged case of the four WebP case modules"""
    rng = np.random.default_rng(9)
    files = [d for _, d in W.taken_cases()] + [d for _, d, _ in W.refused_cases()]
    files += [d for _, _, d in A.all_taken(None)] + [d for _, d, _ in A.refused_cases()]
    files += [d for _, d in L.taken_cases()] + [d for _, d, _ in L.refused_cases()]
    files += [d for _, _, d in N.valid_cases()] + [d for _, d, _ in N.invalid_cases()] + [d for _, d in N.unshared_cases()]
    files += [m for b in W.taken_cases()[:12] for m in W.damaged(b[1], rng, 25)] + [m for b in L.fuzz_bases() for m in W.damaged(b, rng, 20)]
    files += [m for b in A.fuzz_bases() for m in A.damaged(b, rng, 20)] + [d for _, d in N.cut_cases()] + [d for _, d in N.byte_changes(2000)]
    return files


def test_the_probes_share_no_file(K):
    """ke_webpn_probe takes no file ke_webp_probe gives another status than 1 (the chain offers it only those), no file is taken
    by two of webpl / webpa / webpn, and the canvas it reports is Pillow's shape."""
    lib = K._native.load_library()
    files = _all_webp_files()
    st = {kind: _probe(lib, kind, files)[3] for kind in ("webp", "webpl", "webpa", "webpn")}
    took = st["webpn"] == 0
    assert took.sum() >= len(N.valid_cases()) and len(files) > 5000
    assert (st["webp"][took] == 1).all()
    assert (((st["webpl"] == 0).astype(int) + (st["webpa"] == 0) + took) <= 1).all()
    cases = N.valid_cases()
    w, h, c, s = _probe(lib, "webpn", [d for _, _, d in cases])
    for k, (_, name, data) in enumerate(cases):
        assert s[k] == 0 and (h[k], w[k], c[k]) == N.pillow_pixels(data).shape, name


def test_caveats_of_the_built_library(K):
    lib = K._native.load_library()
    cases = [(n, d) for f, n, d in N.valid_cases() if f in ("meta", "placed")]
    files = [d for _, d in cases]
    flat = np.frombuffer(b"".join(files) + b"\0", np.uint8)
    sizes = np.array([len(f) for f in files], np.uint64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    flags = np.zeros(len(files), np.int32)
    lib.ke_webpn_caveats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    assert lib.ke_webpn_caveats(flat.ctypes.data, offsets.ctypes.data, sizes.ctypes.data, len(files), flags.ctypes.data) == 0
    for (name, data), got in zip(cases, flags.tolist()):
        assert got == (1 if N.with_meta(data) else 0) | (2 if data[20] & N.ALPHA else 0), name
    assert set(flags.tolist()) == {0, 1, 2, 3}


def test_enabled_kinds(K, monkeypatch):
    """webpn is offered files by the hashing seam only, with KE_GPU_WEBP_ANIMATED=1 and KE_GPU_WEBP not "0"; never by the refine
    seams, also with every opt-in set.  It is the last row and the last of webp's follow-ups."""
    from kobato_eyes_amd import formats as F

    kinds = lambda seam: [k for k, _ in F.enabled_kinds(seam)]          # noqa: E731
    for f in F.FORMATS:
        monkeypatch.delenv(f.off_switch, raising=False)
        if f.opt_in:
            monkeypatch.delenv(f.opt_in, raising=False)
    monkeypatch.delenv("KE_GPU_REFINE_DECODE", raising=False)
    assert all("webpn" not in kinds(s) for s in ("hash", "refine", "refine_parallel"))
    monkeypatch.setenv("KE_GPU_WEBP_ANIMATED", "1")
    assert kinds("hash")[-2:] == ["webp", "webpn"] and dict(F.enabled_kinds("hash"))["webpn"] == (".webp",)
    assert "webpn" not in kinds("refine") and "webpn" not in kinds("refine_parallel")
    monkeypatch.setenv("KE_GPU_WEBP", "0")
    assert "webpn" not in kinds("hash")
    monkeypatch.setenv("KE_GPU_WEBP", "1")
    monkeypatch.setenv("KE_GPU_WEBP_ANIMATED", "0")
    assert "webpn" not in kinds("hash")
    for f in F.FORMATS:
        if f.opt_in:
            monkeypatch.setenv(f.opt_in, "1")
    assert kinds("hash")[-4:] == ["webp", "webpl", "webpa", "webpn"]
    assert "webpn" not in kinds("refine") and "webpn" not in kinds("refine_parallel") and "webpa" in kinds("refine")
    assert F.follow_ups("webp") == ("webpl", "webpa", "webpn") and F.KINDS[-1] == "webpn" and "webpn" not in F.BASE_KINDS
    row = F.FORMATS[-1]
    assert row.hash_only and [f.kind for f in F.FORMATS if f.hash_only] == ["webpn"]
    assert (row.off_switch, row.opt_in, row.follows, row.luma_only, row.rgba_leave, row.luma_leave) == \
        ("KE_GPU_WEBP", "KE_GPU_WEBP_ANIMATED", "webp", False, None, F.CAVEAT_ORIENTATION)
