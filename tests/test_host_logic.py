"""CPU tests of the host side: the C-ABI library loads and exports every declared symbol, the
drop-in dataclasses / row parsing / cluster assembly reproduce the reference's goldens, the
product refuses to run without a GPU, and the N>1 sharding logic works under gloo."""
from __future__ import annotations

import os
import re
import sqlite3
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def K():
    if not os.path.exists(os.path.join(ROOT, "kobato-eyes_amd", "libkeyes_hip.so")):
        subprocess.check_call(["bash", os.path.join(ROOT, "kobato-eyes_amd", "build.sh")])
    import kobato_eyes_amd

    return kobato_eyes_amd


def test_library_exports_every_declared_symbol(K):
    header = open(os.path.join(ROOT, "include", "keyes.h")).read()
    declared = set(re.findall(r"\b(ke_[a-z0-9_]+)\s*\(", header)) - {"ke_ctx"}
    lib = K._native.load_library()
    assert declared == set(K._native.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.ke_abi_version() == 1


def test_format_table_offers_each_seam_the_kinds_it_always_did(K, monkeypatch):
    """formats.enabled_kinds against the literals the three seams used to carry (fastsig's *_SUFFIXES / GPU_KINDS / FOLLOW_UPS,
    refine's ladder of KE_GPU_* variables, refine_parallel's _GPU_SUFFIXES and its kind -> variable dict), written out here:
    the same kinds, in the same order, with the same suffix tuples, for nothing set, each off-switch alone, each opt-in alone,
    and an opt-in whose base decoder is switched off.  refine never offers gif; refine_parallel runs the base kinds first."""
    from kobato_eyes_amd.formats import enabled_kinds

    suffixes = {"jpeg": (".jpg", ".jpeg", ".jpe", ".jfif"), "png": (".png", ".apng"), "bmp": (".bmp",), "gif": (".gif",),
                "tiff": (".tif", ".tiff"), "tiffc": (".tif", ".tiff"), "webp": (".webp",), "webpl": (".webp",), "webpa": (".webp",)}
    cases = [      # environment, hashing seam, refine, refine_parallel
        ({}, "jpeg png bmp gif tiff webp", "jpeg png bmp tiff webp", "jpeg png bmp gif tiff webp"),
        ({"KE_GPU_JPEG": "0"}, "png bmp gif tiff webp", "png bmp tiff webp", "png bmp gif tiff webp"),
        ({"KE_GPU_PNG": "0"}, "jpeg bmp gif tiff webp", "jpeg bmp tiff webp", "jpeg bmp gif tiff webp"),
        ({"KE_GPU_BMP": "0"}, "jpeg png gif tiff webp", "jpeg png tiff webp", "jpeg png gif tiff webp"),
        ({"KE_GPU_GIF": "0"}, "jpeg png bmp tiff webp", "jpeg png bmp tiff webp", "jpeg png bmp tiff webp"),
        ({"KE_GPU_TIFF": "0"}, "jpeg png bmp gif webp", "jpeg png bmp webp", "jpeg png bmp gif webp"),
        ({"KE_GPU_WEBP": "0"}, "jpeg png bmp gif tiff", "jpeg png bmp tiff", "jpeg png bmp gif tiff"),
        ({"KE_GPU_TIFF_COMPRESSED": "1"}, "jpeg png bmp gif tiff tiffc webp", "jpeg png bmp tiff tiffc webp", "jpeg png bmp gif tiff webp tiffc"),
        ({"KE_GPU_WEBP_LOSSLESS": "1"}, "jpeg png bmp gif tiff webp webpl", "jpeg png bmp tiff webp webpl", "jpeg png bmp gif tiff webp webpl"),
        ({"KE_GPU_WEBP_ALPHA": "1"}, "jpeg png bmp gif tiff webp webpa", "jpeg png bmp tiff webp webpa", "jpeg png bmp gif tiff webp webpa"),
        ({"KE_GPU_TIFF": "0", "KE_GPU_TIFF_COMPRESSED": "1"}, "jpeg png bmp gif webp", "jpeg png bmp webp", "jpeg png bmp gif webp"),
        ({"KE_GPU_REFINE_DECODE": "0"}, "jpeg png bmp gif tiff webp", "", ""),
    ]
    variables = sorted({v for env, *_ in cases for v in env})
    for env, *expected in cases:
        for v in variables:
            monkeypatch.delenv(v, raising=False)
        for v, value in env.items():
            monkeypatch.setenv(v, value)
        for seam, kinds in zip(("hash", "refine", "refine_parallel"), expected):
            assert enabled_kinds(seam) == [(k, suffixes[k]) for k in kinds.split()], (env, seam)


def test_host_side_file_batching_needs_no_gpu(K, tmp_path):
    """ke_host_read_files / ke_host_pack are plain host code (threads, read(2), memcpy): a batch of paths lands back to back
    in the caller's buffer, unreadable or empty files with size 0, and a buffer that is too small is reported, not overrun."""
    import ctypes as C

    lib = K._native.load_library()
    rng = np.random.default_rng(7)
    blobs = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(1, 5000, 700)]
    paths = []
    for k, b in enumerate(blobs):
        p = tmp_path / f"b{k}.bin"
        p.write_bytes(b)
        paths.append(str(p))
    (tmp_path / "empty.bin").write_bytes(b"")
    paths[100:100] = [str(tmp_path / "missing.bin"), str(tmp_path / "empty.bin"), str(tmp_path)]      # a directory, too
    blobs[100:100] = [b"", b"", b""]
    n = len(paths)
    names = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    off, size, needed = np.zeros(n, np.uint64), np.zeros(n, np.uint64), C.c_uint64(0)
    rc = lib.ke_host_read_files(names, n, None, 0, off.ctypes.data, size.ctypes.data, C.byref(needed))
    total = sum(len(b) for b in blobs)
    assert rc == -4 and needed.value == total + 64 and size.tolist() == [len(b) for b in blobs]
    small = np.full(total, 0xAB, np.uint8)
    assert lib.ke_host_read_files(names, n, small.ctypes.data, total, off.ctypes.data, size.ctypes.data, C.byref(needed)) == -4
    assert (small == 0xAB).all()
    buf = np.full(total + 64, 0xAB, np.uint8)
    import resource

    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
    resource.setrlimit(resource.RLIMIT_NOFILE, (min(soft, 128), hard))      # far fewer descriptors than files in the batch
    try:
        assert lib.ke_host_read_files(names, n, buf.ctypes.data, total + 64, off.ctypes.data, size.ctypes.data, C.byref(needed)) == 0
    finally:
        resource.setrlimit(resource.RLIMIT_NOFILE, (soft, hard))
    assert bytes(buf[:total]) == b"".join(blobs) and not buf[total:].any()
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(b) for b in blobs])[:-1]]).tolist()
    # the same bytes from buffers already in memory
    keep = [b for b in blobs if b]
    sizes = np.array([len(b) for b in keep], np.uint64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    dst = np.zeros(total, np.uint8)
    srcs = (C.c_char_p * len(keep))(*keep)
    assert lib.ke_host_pack(dst.ctypes.data, srcs, offs.ctypes.data, sizes.ctypes.data, len(keep)) == 0
    assert bytes(dst) == b"".join(keep)


def test_decode_caveats_follow_the_files_markers(K):
    """ke_jpeg_caveats / ke_png_caveats (host code): the flags say when the reference's loader would turn the image by its EXIF
    orientation or composite its transparency -- checked against what Pillow itself reads from the same bytes."""
    import ctypes as C
    import io

    from PIL import Image, ImageOps

    lib = K._native.load_library()
    arr = (np.arange(24 * 16 * 3) % 251).astype(np.uint8).reshape(16, 24, 3)

    def save(fmt, img=None, **kw):
        b = io.BytesIO()
        (img or Image.fromarray(arr)).save(b, fmt, **kw)
        return b.getvalue()

    def exif(value):
        e = Image.Exif()
        e[0x0112] = value
        return e.tobytes()

    jpegs = [save("JPEG")] + [save("JPEG", exif=exif(v)) for v in range(0, 10)]
    app1 = b"\xff\xe1" + (2 + 6 + 5).to_bytes(2, "big") + b"Exif\0\0" + b"junk!"
    jpegs.append(jpegs[0][:2] + app1 + jpegs[0][2:])             # an EXIF block that cannot be followed
    pngs = [save("PNG"), save("PNG", exif=exif(6)), save("PNG", exif=exif(1)), save("PNG", Image.fromarray(arr).convert("P"), transparency=2),
            save("PNG", Image.fromarray(np.dstack([arr, arr[:, :, :1]]), "RGBA"))]
    for kind, blobs in (("jpeg", jpegs), ("png", pngs)):
        flat = np.frombuffer(b"".join(blobs) + bytes(64), np.uint8)
        sizes = np.array([len(b) for b in blobs], np.uint64)
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
        flags = np.full(len(blobs), -1, np.int32)
        assert getattr(lib, f"ke_{kind}_caveats")(flat.ctypes.data, offs.ctypes.data, sizes.ctypes.data, len(blobs), flags.ctypes.data) == 0
        for k, blob in enumerate(blobs):
            try:
                with Image.open(io.BytesIO(blob)) as im:
                    turned = ImageOps.exif_transpose(im).size != im.size or im.getexif().get(0x0112, 1) in (2, 3, 4)
                    has_exif = "exif" in im.info or bool(im.getexif())
                    transparent = kind == "png" and "transparency" in im.info
            except Exception:
                turned, has_exif, transparent = True, True, False
            if turned:
                assert flags[k] & 1, (kind, k)
            if not has_exif:
                assert not flags[k] & 1, (kind, k)              # nothing to apply: the file may take the GPU decoder
            assert bool(flags[k] & 2) == transparent, (kind, k)


def test_no_cpu_fallback_without_gpu(K):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError):
        K._native.Context(0)
    from PIL import Image

    with pytest.raises(RuntimeError):      # same contract as the reference when cv2 is missing (src/sig/phash.py:35-36)
        K.phash(Image.new("RGB", (64, 64)))


def test_product_never_imports_the_oracle():
    """Nothing under the product package imports, links or opens anything under oracle/."""
    pkg = os.path.join(ROOT, "kobato-eyes_amd")
    pattern = re.compile(r"(from|import)\s+oracle|libkeyes_oracle|keyes_oracle|[\"'/]oracle[/\"']")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h", ".sh")) and f != "dct_table.h":   # generated constants
                text = open(os.path.join(dirpath, f), encoding="utf-8").read()
                assert not pattern.search(text), os.path.join(dirpath, f)


def test_from_row_matches_reference(K):
    rows, expected, bad = G.rows_golden()
    for row, exp in zip(rows, expected):
        f = K.DuplicateFile.from_row(row)
        got = {"file_id": f.file_id, "path": f.path.as_posix(), "size": f.size, "width": f.width, "height": f.height,
               "phash": str(f.phash), "resolution": f.resolution, "extension_priority": f.extension_priority}
        assert got == exp
    for row in bad:
        with pytest.raises(ValueError, match="missing perceptual hash"):
            K.DuplicateFile.from_row(row)


def test_from_row_accepts_sqlite_rows(K):
    conn = sqlite3.connect(":memory:")
    conn.row_factory = sqlite3.Row
    conn.execute("CREATE TABLE t (file_id INTEGER, path TEXT, size INTEGER, width INTEGER, height INTEGER, phash_u64 INTEGER)")
    conn.execute("INSERT INTO t VALUES (7, 'a/b.PNG', 10, 3, 4, -2)")
    f = K.DuplicateFile.from_row(conn.execute("SELECT * FROM t").fetchone())
    assert (f.file_id, f.phash, f.extension_priority, f.resolution) == (7, (1 << 64) - 2, 4, 12)


def test_config_validation(K):
    for kw in ({"band_bits": 0}, {"band_count": 0}, {"hamming_threshold": -1}, {"hamming_threshold": 65},
               {"cosine_threshold": 1.5}):
        with pytest.raises(ValueError):
            K.DuplicateScanConfig(**kw)
    with pytest.raises(AssertionError):
        K.DuplicateScanner(K.DuplicateScanConfig(band_bits=32, band_count=3))
    s = K.DedupSettings.coerce("12", "0.5")
    assert (s.hamming_threshold, s.ssim_threshold) == (12, 0.5)
    s = K.DedupSettings.coerce("x", None)
    assert (s.hamming_threshold, s.ssim_threshold) == (10, 0.92)     # src/core/config/schema.py:186-201
    assert K.DedupSettings.coerce(-4, 1).hamming_threshold == 0


@pytest.mark.parametrize("name", sorted(G.scan_scenarios()))
def test_cluster_assembly_matches_reference(K, name):
    """Edges (from the golden file) -> clusters through the product's host code: union-find in
    libkeyes_hip.so + the reference's keeper / ordering rules."""
    sc = G.scan_scenarios()[name]
    files = [K.DuplicateFile(file_id=f["file_id"], path=Path(f["path"]), size=f["size"], width=f["width"],
                             height=f["height"], phash=f["phash"] & ((1 << 64) - 1)) for f in sc["files"]]
    from kobato_eyes_amd.scanner import DuplicateEdge

    edges = [DuplicateEdge(a, b, h) for a, b, h in sc["edges"]]
    clusters = K.assemble_clusters(files, edges) if edges else []
    got = [{"keeper_id": c.keeper_id, "entries": [[e.file.file_id, e.best_hamming] for e in c.files]} for c in clusters]
    assert got == sc["clusters"]


def test_first_writer_rule_with_duplicate_ids(K):
    """_edges_from_raw resolves duplicate file ids exactly as the reference's dict insertion order does."""
    sc = G.scan_scenarios()["dup_ids_signed"]
    from oracle import oracle as O

    files = [K.DuplicateFile(file_id=f["file_id"], path=Path(f["path"]), size=f["size"], width=f["width"],
                             height=f["height"], phash=f["phash"] & ((1 << 64) - 1)) for f in sc["files"]]
    hashes, ids, _ = G.files_to_arrays(sc["files"])
    raw = O.scan_bruteforce(hashes, threshold=10)          # every (i,j,h,bands) the GPU kernel would emit...
    raw = raw[ids[raw["a"]] != ids[raw["b"]]]              # ...after its same-id test
    scanner = K.DuplicateScanner(K.DuplicateScanConfig(**sc["config"]))
    edges = scanner._edges_from_raw(files, hashes, ids, raw, np.array([0, int(sum(bin(b).count("1") for b in raw["bands"])), len(raw), 0], np.uint64))
    assert sorted([a, b, e.hamming] for (a, b), e in edges.items()) == sc["edges"]


def test_cluster_builder(K):
    M = K.RefinedMatch
    out = K.ClusterBuilder().build([M(1, 2, 0.95, 0.2, True, "ssim"), M(2, 3, 0.93, 0.15, True, "ssim"),
                                    M(4, 5, 0.91, 0.16, True, "ssim"), M(3, 5, 0.5, 0.05, False, "below")])
    assert [c.members for c in out] == [[1, 2, 3], [4, 5]] and [c.representative for c in out] == [1, 4]
    assert [len(c.matches) for c in out] == [2, 1]
    assert K.ClusterBuilder().build([]) == []


def test_signed_wrap_and_upsert(K, tmp_path):
    from kobato_eyes_amd.fastsig import _to_signed64

    assert [_to_signed64(v) for v in (0, (1 << 64) - 1, 1 << 63, (1 << 63) - 1, (1 << 64) + 7)] == [0, -1, -(1 << 63), (1 << 63) - 1, 7]
    db = tmp_path / "s.db"
    conn = sqlite3.connect(db)
    conn.execute("CREATE TABLE signatures (file_id INTEGER PRIMARY KEY, phash_u64 INTEGER NOT NULL, dhash_u64 INTEGER NOT NULL)")
    assert K.bulk_upsert_signatures(conn, [(1, (1 << 64) - 1, 5), (2, 2, 0)]) == 2
    assert K.bulk_upsert_signatures(conn, [(2, 1 << 63, 9)]) == 1
    assert conn.execute("SELECT * FROM signatures ORDER BY file_id").fetchall() == [(1, -1, 5), (2, -(1 << 63), 9)]
    assert K.bulk_upsert_signatures(conn, []) == 0


def test_fastsig_drops_missing_files_and_reports_progress(K, monkeypatch, tmp_path):
    """Progress cadence / cancel semantics of src/core/fastsig.py:86-98 with the GPU hasher stubbed out
    (this is host logic; the hashing itself is covered by the gpu tests)."""
    import kobato_eyes_amd.fastsig as fs
    from PIL import Image

    paths = []
    for k in range(5):
        p = tmp_path / f"i{k}.png"
        Image.new("RGB", (8, 8), (k, k, k)).save(p)
        paths.append((k + 1, str(p)))
    paths.insert(2, (99, str(tmp_path / "missing.png")))
    class FakeStage(fs._Stage):                            # what fastsig._Stage requires, no device behind it
        def __init__(self, device, stage_bytes, max_images):
            self.bufs, self.turn, self.submitted = [np.zeros(4096, np.uint8), np.zeros(4096, np.uint8)], 0, []

        def acquire(self):
            slot = self.turn
            self.turn ^= 1
            return slot, self.bufs[slot]

        def submit(self, slot, offsets, widths, heights, channels):
            assert all(o % 16 == 0 for o in offsets) and list(widths) == [8] * len(offsets) and list(channels) == [3] * len(offsets)
            for o in offsets:                              # the decode threads wrote the pixels where the allocator said
                px = self.bufs[slot][o:o + 192]
                assert len(set(px.tolist())) == 1
            self.submitted.append(len(offsets))
            n = len(offsets)
            return {"phash": np.arange(n, dtype=np.uint64) + np.uint64(1 << 63), "dhash": np.zeros(n, np.uint64), "status": np.zeros(n, np.int32)}

        def wait(self, slot):
            pass

        def hash_files(self, paths, kind):                  # "the GPU decoder refuses every file": all take the Pillow route
            assert kind == "png"
            for p in paths:
                if os.path.exists(p):                       # the missing one: refused like the rest, and Pillow drops it
                    with open(p, "rb") as fh:
                        assert fh.read(4) == b"\x89PNG"
            n = len(paths)
            return np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.ones(n, np.int32)

        def hash_one(self, arr):
            return (1 << 63, 0)

    monkeypatch.setattr(fs, "_make_stage", FakeStage)
    seen = []
    out = fs.compute_signatures_mp(paths, max_workers=2, chunksize=4, progress=lambda d, t: seen.append((d, t)))
    assert [r[0] for r in out] == [1, 2, 3, 4, 5] and seen == [(6, 6)]
    assert all(r[1] < 0 for r in out)                      # stored signed
    full = out
    calls = {"n": 0}

    def cancel():
        calls["n"] += 1
        return calls["n"] > 6

    # the callback is asked between the chunks of the Pillow route and before each GPU decode call (4 times for these six
    # files) and then once per result, as the reference does (src/core/fastsig.py:86-90): a prefix comes back
    out = fs.compute_signatures_mp(paths, max_workers=2, chunksize=4, cancel_fn=cancel)
    assert 0 < len(out) < len(full) and out == full[:len(out)]
    calls["n"] = 0
    stopped_early = fs.compute_signatures_mp(paths, max_workers=2, chunksize=4, cancel_fn=lambda: True)
    assert stopped_early == []                             # asked before any work: nothing decoded, nothing returned


def test_fastsig_progress_cadence_over_whole_batches(K, monkeypatch):
    """Without a cancel callback results are taken a GPU batch at a time; progress still fires at every 200th file and at
    the end (src/core/fastsig.py:95-98), failures are still omitted."""
    import kobato_eyes_amd.fastsig as fs

    class FakePipeline:
        def __init__(self, tasks, workers, chunk, device, cancel_fn=None):
            self.tasks = tasks

        def run_batches(self):
            for lo in range(0, len(self.tasks), 128):
                fids = np.array([t[0] for t in self.tasks[lo:lo + 128]], np.int64)
                yield fids, -fids, fids.copy(), fids % 50 != 0

    monkeypatch.setattr(fs, "_Pipeline", FakePipeline)
    for total, marks in ((450, [200, 400, 450]), (400, [200, 400]), (199, [199]), (128, [128])):
        seen = []
        rows = fs.compute_signatures_mp([(k, f"f{k}") for k in range(1, total + 1)], progress=lambda d, t: seen.append((d, t)))
        assert seen == [(m, total) for m in marks]
        assert rows == [(k, -k, k) for k in range(1, total + 1) if k % 50]


_GLOO_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from kobato_eyes_amd.distributed import allgather_hashes, allgather_edge_buffers, gather_edges, owned_indices, interleave_gathered
from kobato_eyes_amd import _native
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % sys.argv[2], rank=int(sys.argv[3]), world_size=2)
rank, world, n = dist.get_rank(), 2, 1001
table = (np.arange(n, dtype=np.int64) * 7919) ^ 0x5555
mine = owned_indices(n, rank, world)
local = torch.from_numpy(table[mine].copy())
full = allgather_hashes(local, n)
assert np.array_equal(full.numpy(), table), "all-gather did not restore corpus order"
edges = np.zeros(3 + rank, _native.EDGE_DTYPE); edges["a"] = rank; edges["b"] = np.arange(len(edges)) + 10
merged = gather_edges(edges)
assert len(merged) == 7 and sorted(merged["a"].tolist()) == [0, 0, 0, 1, 1, 1, 1]
buf = torch.zeros(24 * 8, dtype=torch.uint8); buf[: edges.nbytes] = torch.from_numpy(edges.view(np.uint8).copy())
raw, counts = allgather_edge_buffers(buf, len(edges))
m2 = raw.view(_native.EDGE_DTYPE)
assert counts == [3, 4] and m2["a"].tolist() == [0, 0, 0, 1, 1, 1, 1] and m2["b"].tolist() == [10, 11, 12, 10, 11, 12, 13]
# one rank holds more edges than the fixed-width record carries: the second (full-width) all-gather, then the
# record grows and the next merge is a single collective again
big = np.zeros(1500 if rank == 1 else 2, _native.EDGE_DTYPE); big["a"] = rank; big["b"] = np.arange(len(big))
bbuf = torch.from_numpy(big.view(np.uint8).copy())
for _ in range(2):
    raw, counts = allgather_edge_buffers(bbuf, len(big))
    m3 = raw.view(_native.EDGE_DTYPE)
    assert counts == [2, 1500] and m3["a"].tolist() == [0, 0] + [1] * 1500 and m3["b"].tolist() == [0, 1] + list(range(1500))
raw, counts = allgather_edge_buffers(torch.zeros(0, dtype=torch.uint8), 0)
assert counts == [0, 0] and len(raw) == 0
parts = [table[owned_indices(n, r, world)] for r in range(world)]
assert np.array_equal(interleave_gathered(parts, n), table)
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_sharding_helpers_world_size_2_gloo(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_GLOO_WORKER)
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(port), str(r)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=180)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o


def test_decode_normalisation_matches_reference(K, tmp_path):
    """kobato_eyes_amd.image_io.safe_load_image against what the reference's utils.image_io.safe_load_image
    returned for the same files (tests/golden/image_io_golden.json): mode, size and every pixel."""
    import hashlib
    import warnings

    from kobato_eyes_amd.image_io import safe_load_image

    golden = G.image_io_golden()
    seen = 0
    for name, path, kwargs in G.write_image_io_files(tmp_path):
        exp = golden[name]
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                img = safe_load_image(path, **kwargs)
        except Exception as exc:
            assert exp == {"raises": type(exc).__name__}, name
            seen += 1
            continue
        if exp is None:
            assert img is None, name
        else:
            assert img is not None and "raises" not in exp, name
            got = {"mode": img.mode, "size": list(img.size), "sha256": hashlib.sha256(img.tobytes()).hexdigest()}
            assert got == exp, name
        seen += 1
    assert seen == len(golden) >= 20


def test_cluster_maintenance_matches_reference(K):
    """rebuild_clusters_after_removal / cluster_hamming_score / default_checked_entries against the reference's
    ui.dup_cluster_update and ui.dup_tree_state run on the same clusters (tests/golden/cluster_update_golden.json)."""
    import json

    from oracle import oracle as O

    with open(os.path.join(G.GOLDEN, "cluster_update_golden.json")) as fh:
        g = json.load(fh)
    ext = ("png", "jpg", "webp", "jpeg", "bmp", "tif")
    files = {i + 1: K.DuplicateFile(file_id=i + 1, path=Path(f"dir{i % 3}/img_{i:07d}.{ext[i % 6]}"), size=1000 + (i % 7),
                                    width=512 - (i % 5), height=512, phash=int(hv)) for i, hv in enumerate(O.synth_hashes(1000))}
    clusters = [K.DuplicateCluster(files=[K.DuplicateClusterEntry(files[fid], best) for fid, best in entries], keeper_id=keeper)
                for keeper, entries in g["clusters"]]
    enc = lambda cs: [[c.keeper_id, [[e.file.file_id, e.best_hamming] for e in c.files]] for c in cs]
    for case in g["removals"]:
        assert enc(K.rebuild_clusters_after_removal(clusters, set(case["removed"]))) == case["result"]
    assert [K.cluster_hamming_score(c) for c in clusters] == g["hamming_score"]
    assert [[e.file.file_id for e in K.default_checked_entries(c)] for c in clusters] == g["default_checked"]
    assert K.rebuild_cluster_after_removal(clusters[0], {e.file.file_id for e in clusters[0].files[1:]}) is None
    assert K.choose_keeper(clusters[0].files) == clusters[0].keeper_id


def test_batches_read_ahead_reach_the_decoders_in_their_own_order(tmp_path, monkeypatch):
    """fastsig._Pipeline with a stage that reads files itself (the shape of _GpuStage: read_ahead / hash_ahead / hash_files):
    the next batch is read while the current one is hashed, JPEG files first and PNG files after them in the buffer, each
    kind handed its own slice; a batch whose read-ahead found no buffer goes through hash_files; every buffer comes back, also
    when the run is given up half way.  No device: the 'hashes' are numbers taken from the file names."""
    from kobato_eyes_amd import fastsig as fs

    items = []
    for k in range(23):
        p = tmp_path / f"f{k:03d}.{'png' if k % 3 == 0 else 'jpg'}"
        p.write_bytes(b"x")
        items.append((1000 + k, str(p)))
    log = {"ahead": 0, "direct": 0, "released": 0, "taken": 0}

    class Held:
        def __init__(self, paths):
            self.paths = paths

        def release(self):
            log["released"] += 1

    def numbers(paths, kind):
        assert all(p.endswith("png" if kind == "png" else "jpg") for p in paths)
        n = np.array([int(os.path.basename(p)[1:4]) for p in paths], np.uint64)
        return n, n + np.uint64(500), np.where(n % 5 == 4, 1, 0).astype(np.int32)     # every fifth file is left to Pillow

    class Stage(fs._Stage):
        def __init__(self, device, stage_bytes, max_images):
            self.buf = np.zeros(1 << 16, np.uint8)

        def acquire(self):
            return 0, self.buf

        def submit(self, slot, offsets, widths, heights, channels):
            raise AssertionError("nothing decodes here: the files are not images")

        def wait(self, slot):
            pass

        def hash_one(self, arr):
            return None

        def read_ahead(self, paths, spans=()):
            jpegs = sum(p.endswith("jpg") for p in paths)
            assert tuple(spans) == (("jpeg", 0, jpegs), ("png", jpegs, len(paths)), ("bmp", len(paths), len(paths)), ("gif", len(paths), len(paths)), ("tiff", len(paths), len(paths)))
            log["taken"] += 1
            if log["taken"] == 2:                              # "both buffers taken": this batch is read inside the call
                return None
            log["ahead"] += 1
            return Held(list(paths))

        def hash_ahead(self, held, lo, hi, kind="jpeg"):
            return numbers(held.paths[lo:hi], kind)

        def hash_files(self, paths, kind="jpeg"):
            log["direct"] += 1
            return numbers(paths, kind)

    monkeypatch.setattr(fs, "_make_stage", Stage)
    monkeypatch.setenv("KE_GPU_BATCH", "8")
    monkeypatch.setenv("KE_DECODE_PROCESSES", "0")
    rows = fs.compute_signatures_mp(items, max_workers=2, chunksize=8)
    want = [(1000 + k, k, k + 500) for k in range(23) if k % 5 != 4]          # the refused ones are not images: dropped
    assert rows == want
    assert log["ahead"] == 2 and log["released"] == 2 and log["direct"] == 2   # three batches: one of them jpeg + png direct
    batches = fs._Pipeline(items, 2, 8, 0).run_batches()
    next(batches)
    batches.close()
    assert log["released"] == log["ahead"]


_CHAIN_EXT = ("jpg", "png", "gif", "tif", "webp")                    # file k has suffix _CHAIN_EXT[k % 5]
_CHAIN_BASE = {"jpg": "jpeg", "png": "png", "gif": "gif", "tif": "tiff", "webp": "webp"}
_CHAIN_REFUSED = {15: "jpeg", 26: "png", 7: "gif", 13: "tiff", 24: "webp"}          # status 2 from the suffix's own decoder
_CHAIN_LEFT = {"jpeg": {30}, "png": set(), "gif": set(), "tiff": {8, 23, 33}, "webp": {4, 14, 19, 29, 39}}   # status 1 from it
_CHAIN_TAKES = {"tiffc": {8, 33}, "webpl": {4, 29}, "webpa": {14, 39}}               # 23 and 19: nobody takes them
_CHAIN_FOLLOWS = {"tiffc": "tiff", "webpl": "webp", "webpa": "webp"}
_CHAIN_BIG_PNG = 21                                                  # the PNG file the read-ahead reports as 10 MB


def _chain_status(k: int, kind: str) -> int:
    if kind in _CHAIN_TAKES:
        return 0 if k in _CHAIN_TAKES[kind] else 1
    return 2 if k in _CHAIN_REFUSED else 1 if k in _CHAIN_LEFT[kind] else 0


@pytest.mark.parametrize("route", ["ahead", "ahead_png_skip", "paths"])
def test_follow_up_decoders_are_offered_what_their_base_left_on_every_route(tmp_path, monkeypatch, route):
    """fastsig._Pipeline's chain base decoder -> follow-ups (formats.follow_ups) with a stand-in stage, once per way the files
    reach it: a read-ahead buffer (``hash_ahead`` with a ``skip`` mask; one batch finds no buffer and goes through
    ``hash_files``) and paths (``hash_files`` with a filtered list).  File k's only
    byte is k, its 'hashes' are (k, k + 500), and its status is a function of k and the kind (_chain_status): every follow-up
    call must be handed exactly the files still at status 1 after the decoders before it -- never one its base gave 0 or 2 --,
    the rows are those somebody took, every buffer comes back, and a PNG file that ``_largest_for_pillow`` moves to the Pillow
    side is neither hashed by the stage nor returned twice."""
    from kobato_eyes_amd import fastsig as fs

    n_files = 40
    items = []
    for k in range(n_files):
        p = tmp_path / f"f{k:03d}.{_CHAIN_EXT[k % 5]}"
        p.write_bytes(bytes([k]))
        items.append((1000 + k, str(p)))
    for v in ("KE_GPU_JPEG", "KE_GPU_PNG", "KE_GPU_BMP", "KE_GPU_GIF", "KE_GPU_TIFF", "KE_GPU_WEBP", "KE_READ_AHEAD"):
        monkeypatch.delenv(v, raising=False)
    for v in ("KE_GPU_TIFF_COMPRESSED", "KE_GPU_WEBP_LOSSLESS", "KE_GPU_WEBP_ALPHA"):
        monkeypatch.setenv(v, "1")
    monkeypatch.setenv("KE_GPU_BATCH", "8")
    monkeypatch.setenv("KE_DECODE_PROCESSES", "0")
    monkeypatch.setenv("KE_PNG_GPU_US_PER_BYTE", "0.9" if route == "ahead_png_skip" else "0")
    monkeypatch.setenv("KE_GIF_GPU_US_PER_BYTE", "0")
    monkeypatch.setenv("KE_DECODE_POOL_START_S", "0")
    log = {"reads": 0, "held": 0, "released": 0, "offers": [], "hashed": [], "routes": set()}

    def number(path: str) -> int:
        return int(os.path.basename(path)[1:4])

    def answer(ks, kind, how):
        """What the decoder of ``kind`` says about files ``ks``; a follow-up's call is written down, and checked file by file."""
        ks = [int(k) for k in ks]
        log["routes"].add(how)
        base = _CHAIN_FOLLOWS.get(kind, kind)
        assert all(_CHAIN_BASE[_CHAIN_EXT[k % 5]] == base for k in ks), (kind, ks)
        if kind in _CHAIN_FOLLOWS:
            assert ks and all(_chain_status(k, base) == 1 for k in ks), (kind, ks)
            log["offers"].append((kind, ks))
        log["hashed"] += ks
        num = np.array(ks, np.uint64)
        return num, num + np.uint64(500), np.array([_chain_status(k, kind) for k in ks], np.int32)

    class Held:
        def __init__(self, paths, spans):
            self.paths = paths
            self.sizes = np.array([10_000_000 if number(p) == _CHAIN_BIG_PNG else 1 for p in paths], np.uint64)
            self.probed = {(kind, lo, hi): (np.full(hi - lo, 2048, np.int32), np.full(hi - lo, 2048, np.int32), np.full(hi - lo, 3, np.int32),
                                            np.zeros(hi - lo, np.int32)) for kind, lo, hi in spans if hi > lo}   # 12 MB each for Pillow
            self.out = False

        def release(self):
            assert not self.out
            self.out = True
            log["released"] += 1

    class Stage(fs._Stage):
        def __init__(self, device, stage_bytes, max_images):
            self.buf = np.zeros(1 << 16, np.uint8)

        def acquire(self):
            return 0, self.buf

        def submit(self, slot, offsets, widths, heights, channels):
            raise AssertionError("nothing decodes here: the files are not images")

        def wait(self, slot):
            pass

        def hash_one(self, arr):
            return None

        def hash_files(self, paths, kind="jpeg"):
            return answer([number(p) for p in paths], kind, "paths")

    def read_ahead(self, paths, spans=()):
        log["reads"] += 1
        if log["reads"] == 2:                                  # "both buffers taken": this batch is read inside the call
            return None
        log["held"] += 1
        return Held(list(paths), spans)

    def hash_ahead(self, held, lo, hi, kind="jpeg", **more):
        assert not held.out and set(more) <= {"skip"}
        ks = np.array([number(p) for p in held.paths[lo:hi]], np.int64)
        if "skip" not in more:
            return answer(ks, kind, "ahead")
        skip = np.asarray(more["skip"])                        # handed over only when there is a mask
        assert skip.dtype == bool and skip.shape == ks.shape
        p, d, st = (np.zeros(len(ks), np.uint64), np.zeros(len(ks), np.uint64), np.ones(len(ks), np.int32))
        p[~skip], d[~skip], st[~skip] = answer(ks[~skip], kind, "ahead")
        return p, d, st

    if route != "paths":
        Stage.read_ahead, Stage.hash_ahead = read_ahead, hash_ahead
    monkeypatch.setattr(fs, "_make_stage", Stage)
    rows = fs.compute_signatures_mp(items, max_workers=2, chunksize=8)

    moved = {_CHAIN_BIG_PNG} if route == "ahead_png_skip" else set()
    taken = set().union(*_CHAIN_TAKES.values())
    want = [(1000 + k, k, k + 500) for k in range(n_files)
            if k not in moved and (k in taken or _chain_status(k, _CHAIN_BASE[_CHAIN_EXT[k % 5]]) == 0)]
    assert rows == want                                        # what nobody took is no image: Pillow drops it
    offers = []
    for lo in range(0, n_files, 8):                            # per batch: tiff's follow-up, then webp's two in their order
        batch = set(range(lo, lo + 8))
        for kind, ks in (("tiffc", _CHAIN_LEFT["tiff"]), ("webpl", _CHAIN_LEFT["webp"]),
                         ("webpa", _CHAIN_LEFT["webp"] - _CHAIN_TAKES["webpl"])):
            if ks & batch:
                offers.append((kind, sorted(ks & batch)))
    assert log["offers"] == offers
    assert not moved & set(log["hashed"]) and len({r[0] for r in rows}) == len(rows)
    assert sorted(k for k in log["hashed"] if k not in set().union(*_CHAIN_LEFT.values())) == \
        sorted(set(range(n_files)) - moved - set().union(*_CHAIN_LEFT.values()))      # every other file: offered once, to its base
    assert log["routes"] == {"ahead": {"ahead", "paths"}, "ahead_png_skip": {"ahead", "paths"}, "paths": {"paths"}}[route]
    if route in ("ahead", "ahead_png_skip"):
        assert log["reads"] == 5 and log["held"] == 4 and log["released"] == 4
    else:
        assert log["reads"] == log["released"] == 0


def test_failed_gpu_call_leaves_to_pillow_only_what_pillow_does_not_have_yet(tmp_path, monkeypatch):
    """A GPU decode call that fails (``hash_ahead`` raises for PNG) on batches of which the cost split has already given one
    file to the Pillow share: every file reaches ``_decode_with_pillow`` exactly once -- the moved one with the share, the
    rest after the failure -- and the rows are those of a run in which Pillow decodes everything.  Twelve real 8 x 8 PNG files
    of colour (k, k, k) in batches of eight; the stand-in's 'hashes' are (k, k + 500), read from the pixels that arrived in
    the staging buffer; files 5 and 9 are reported as 10 MB of 2048 x 2048 x 3, which the split moves (one per batch)."""
    from kobato_eyes_amd import fastsig as fs
    from PIL import Image

    items = []
    for k in range(12):
        p = tmp_path / f"f{k:03d}.png"
        Image.new("RGB", (8, 8), (k, k, k)).save(p)
        items.append((1000 + k, str(p)))
    big = {5, 9}
    log = {"held": 0, "released": 0, "failed": 0}

    class Held:
        def __init__(self, paths, spans):
            self.sizes = np.array([10_000_000 if int(os.path.basename(p)[1:4]) in big else 1 for p in paths], np.uint64)
            self.probed = {(kind, lo, hi): (np.full(hi - lo, 2048, np.int32), np.full(hi - lo, 2048, np.int32), np.full(hi - lo, 3, np.int32),
                                            np.zeros(hi - lo, np.int32)) for kind, lo, hi in spans if hi > lo}
            log["held"] += 1

        def release(self):
            log["released"] += 1

    class Stage(fs._Stage):
        def __init__(self, device, stage_bytes, max_images):
            self.bufs, self.turn = [np.zeros(4096, np.uint8), np.zeros(4096, np.uint8)], 0

        def acquire(self):
            self.turn ^= 1
            return self.turn, self.bufs[self.turn]

        def submit(self, slot, offsets, widths, heights, channels):
            k = np.array([self.bufs[slot][o] for o in offsets], np.uint64)
            return {"phash": k, "dhash": k + np.uint64(500), "status": np.zeros(len(k), np.int32)}

        def wait(self, slot):
            pass

        def hash_one(self, arr):
            return None

        def read_ahead(self, paths, spans=()):
            return Held(paths, spans)

        def hash_ahead(self, held, lo, hi, kind, skip=None):
            assert kind == "png"
            log["failed"] += 1
            raise RuntimeError("no room on the device for this batch")

    asked = []
    inner = fs._Pipeline._decode_with_pillow

    def spy(self, todo, out):
        asked.extend(todo)
        return inner(self, todo, out)

    for v in ("KE_GPU_PNG", "KE_READ_AHEAD", "KE_PNG_GPU_US_PER_BYTE", "KE_PILLOW_MB_PER_S"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("KE_GPU_BATCH", "8")
    monkeypatch.setenv("KE_DECODE_POOL_START_S", "0")
    monkeypatch.setattr(fs, "_make_stage", Stage)
    monkeypatch.setattr(fs._Pipeline, "_decode_with_pillow", spy)
    rows = fs.compute_signatures_mp(items, max_workers=2, chunksize=8)
    assert log["failed"] == 2 and log["held"] == log["released"] == 2
    assert sorted(asked) == list(range(12)), asked             # nobody twice: not the files the Pillow share had already
    assert rows == [(1000 + k, k, k + 500) for k in range(12)]
    monkeypatch.setenv("KE_GPU_PNG", "0")                      # Pillow alone
    assert fs.compute_signatures_mp(items, max_workers=2, chunksize=8) == rows and log["failed"] == 2


def test_batch_reads_give_their_buffer_back_once():
    """_BatchReads.release() however often: the read-ahead buffer is released once, and a batch without one has nothing to do."""
    from kobato_eyes_amd.fastsig import _BatchReads

    class Held:
        released = 0

        def release(self):
            self.released += 1

    held = Held()
    reads = _BatchReads({}, {}, held)
    reads.release()
    reads.release()
    assert held.released == 1 and reads.ahead is None
    _BatchReads({}, {}).release()


def _png_for_pillow_as_the_pipeline_carried_it(workers, pools, held, lo, hi, kind="png"):
    """_Pipeline._png_for_pillow before fastsig._largest_for_pillow, restated literally (``workers`` / ``pools`` for
    ``self.workers`` / the module's ``_pools``)."""
    gpu_rate = float(os.environ.get("KE_PNG_GPU_US_PER_BYTE", "0.9") if kind == "png" else os.environ.get("KE_GIF_GPU_US_PER_BYTE", "0.75")) * 1e-6
    if gpu_rate <= 0.0:
        return None
    known = getattr(held, "probed", {}).get((kind, lo, hi))
    if known is None:
        return None
    w, h, c, st = known
    sizes = np.asarray(held.sizes[lo:hi], np.float64)
    decoded = np.where(st == 0, w.astype(np.float64) * h * c, 0.0)
    n = len(sizes)
    if n == 0:
        return None
    cpu_rate = 1.0 / (max(1, workers) * float(os.environ.get("KE_PILLOW_MB_PER_S", "250")) * 1e6)
    order = np.argsort(-np.where(st == 0, sizes, 0.0), kind="stable")
    longest_left = np.concatenate([np.where(st == 0, sizes, 0.0)[order] * gpu_rate + 4e-3, [0.0]])
    moved = np.concatenate([[0.0], np.cumsum(decoded[order]) * cpu_rate])
    if workers not in pools:
        moved[1:] += float(os.environ.get("KE_DECODE_POOL_START_S", "1.5"))
    k = int(np.argmin(np.maximum(longest_left, moved)))
    if k == 0:
        return None
    mask = np.zeros(n, bool)
    mask[order[:k]] = True
    return mask


def test_cost_split_function_moves_the_files_the_pipeline_method_moved(monkeypatch):
    """fastsig._largest_for_pillow, fed from _Knobs and _SPLIT_RATES as the pipeline feeds it, against the method it replaced
    on 2 000 random spans (n = 0 .. 40, statuses from {0, 1, 2} -- also all refused --, compressed sizes 1 B .. 50 MB, 1 .. 16
    workers, decoder processes started or not, both kinds, a GPU rate of 0 and headers nobody parsed among the settings): the same
    mask element for element, or None from both."""
    from types import SimpleNamespace

    from kobato_eyes_amd import fastsig as fs

    assert fs._SPLIT_RATES == {"png": ("KE_PNG_GPU_US_PER_BYTE", "0.9"), "gif": ("KE_GIF_GPU_US_PER_BYTE", "0.75")}
    settings = [{}, {"KE_PNG_GPU_US_PER_BYTE": "0"}, {"KE_GIF_GPU_US_PER_BYTE": "0", "KE_DECODE_POOL_START_S": "0"},
                {"KE_PNG_GPU_US_PER_BYTE": "0.05", "KE_GIF_GPU_US_PER_BYTE": "3", "KE_PILLOW_MB_PER_S": "40"},
                {"KE_PILLOW_MB_PER_S": "1000", "KE_DECODE_POOL_START_S": "0.01"}]
    rng = np.random.default_rng(20261019)
    moved_some = 0
    for trial in range(2000):
        if trial % 400 == 0:
            for v in ("KE_PNG_GPU_US_PER_BYTE", "KE_GIF_GPU_US_PER_BYTE", "KE_PILLOW_MB_PER_S", "KE_DECODE_POOL_START_S"):
                monkeypatch.delenv(v, raising=False)
            for v, text in settings[trial // 400].items():
                monkeypatch.setenv(v, text)
            knobs = fs._Knobs.read()
        n = trial % 400 if trial % 400 < 2 else int(rng.integers(0, 41))
        kind = ("png", "gif")[int(rng.integers(0, 2))]
        workers, started = int(rng.integers(1, 17)), bool(rng.integers(0, 2))
        lo = int(rng.integers(0, 5))
        sizes = np.floor(np.exp(rng.uniform(0.0, np.log(50e6), lo + n + 3))).astype(np.uint64)
        w, h = rng.integers(1, 4097, n).astype(np.int32), rng.integers(1, 4097, n).astype(np.int32)
        c = rng.choice([1, 3, 4], n).astype(np.int32)
        st = (np.full(n, rng.integers(1, 3)) if trial % 7 == 0 else rng.choice([0, 0, 0, 1, 2], n)).astype(np.int32)
        probed = None if trial % 11 == 0 else (w, h, c, st)
        held = SimpleNamespace(sizes=sizes, probed={} if probed is None else {(kind, lo, lo + n): probed})
        want = _png_for_pillow_as_the_pipeline_carried_it(workers, {workers: None} if started else {}, held, lo, lo + n, kind)
        got = fs._largest_for_pillow(sizes[lo:lo + n], probed, knobs.gpu_s_per_byte[kind],
                                     1.0 / (max(1, workers) * knobs.pillow_mb_per_s * 1e6), 0.0 if started else knobs.pool_start_s)
        assert (got is None and want is None) or (got.dtype == bool and np.array_equal(got, want)), trial
        moved_some += want is not None
    assert moved_some > 200                                    # the comparison is not one of None with None


def _grouped_layout_as_decode_files_owned_wrote_it(w, h, c, st):
    """The by_shape loop Context.decode_files_owned carried before _native.lay_out, restated literally."""
    n = len(w)
    nbytes = np.where(st == 0, w.astype(np.int64) * h * c, 0)
    out_off = np.zeros(n, np.uint64)
    order = np.lexsort((w, h, c, st != 0))
    sorted_bytes = nbytes[order]
    key = np.stack([w[order], h[order], c[order]], 1)
    new_group = np.ones(n, bool)
    new_group[1:] = (key[1:] != key[:-1]).any(1)
    starts = np.zeros(n, np.int64)
    at = 0
    for k in range(n):
        if new_group[k]:
            at = (at + 15) & ~15
        starts[k] = at
        at += int(sorted_bytes[k])
    out_off[order] = starts.astype(np.uint64)
    out_off[nbytes == 0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return out_off, at


def _grouped_layout_as_normalise_rgb_wrote_it(ow, oh):
    """The by_shape loop Context.normalise_rgb carried before _native.lay_out, restated literally."""
    nbytes = ow.astype(np.int64) * oh * 3
    do = np.zeros(len(ow), np.uint64)
    order = np.lexsort((oh, ow))
    at, prev = 0, None
    for k in order.tolist():
        shape = (int(ow[k]), int(oh[k]))
        if shape != prev:
            at, prev = (at + 15) & ~15, shape
        do[k] = at
        at += int(nbytes[k])
    return do, at


def test_one_layout_function_lays_groups_out_as_both_loops_did():
    """_native.lay_out against the two per-image loops it replaced, on 2 000 random batches (n = 0 .. 40, shapes from at most
    four values so that groups form, refused files, files of no bytes): the same offsets, NOT_LAID marks and totals, byte for
    byte, in decode_files_owned's ordering and in normalise_rgb's; the plain form is 16-byte slots in input order; and
    runs_laid_out returns the groups the layout made, in buffer order."""
    from kobato_eyes_amd._native import NOT_LAID, lay_out, runs_laid_out

    assert NOT_LAID == np.uint64(0xFFFFFFFFFFFFFFFF)
    rng = np.random.default_rng(20260611)
    for trial in range(2000):
        n = trial if trial < 2 else int(rng.integers(0, 41))
        values = rng.choice([0, 1, 3, 5, 7, 8, 16, 17, 33], size=int(rng.integers(1, 5)))
        w, h = rng.choice(values, n).astype(np.int32), rng.choice(values, n).astype(np.int32)
        c = rng.choice([1, 3, 4], n).astype(np.int32)
        st = rng.choice([0, 0, 0, 1, 2], n).astype(np.int32)
        nbytes = np.where(st == 0, w.astype(np.int64) * h * c, 0)
        off, total = lay_out(nbytes, (w, h, c), st != 0)
        want_off, want_total = _grouped_layout_as_decode_files_owned_wrote_it(w, h, c, st)
        assert off.dtype == np.uint64 and np.array_equal(off, want_off) and total == want_total, trial
        if total:                                              # the groups back: whole, of one shape, back to back, in buffer order
            runs = runs_laid_out(off, (w, h, c))
            assert sorted(np.concatenate(runs).tolist()) == np.nonzero(nbytes)[0].tolist()
            shapes = [(int(w[r[0]]), int(h[r[0]]), int(c[r[0]])) for r in runs]
            assert len(set(shapes)) == len(shapes) and all(off[r[0]] % 16 == 0 for r in runs)
            for r, (ww, hh, cc) in zip(runs, shapes):
                assert (w[r] == ww).all() and (h[r] == hh).all() and (c[r] == cc).all()
                assert np.array_equal(off[r], off[r[0]] + np.arange(len(r), dtype=np.uint64) * np.uint64(ww * hh * cc))
            assert [int(off[r[0]]) for r in runs] == sorted(int(off[r[0]]) for r in runs)
        off, total = lay_out(w.astype(np.int64) * h * 3, (h, w))
        want_off, want_total = _grouped_layout_as_normalise_rgb_wrote_it(w, h)
        assert np.array_equal(off, want_off) and total == want_total, trial
        if n and (w * h > 0).all():
            runs = runs_laid_out(off, (w, h))
            assert np.array_equal(np.concatenate(runs), np.argsort(off, kind="stable"))
            assert all(len({(int(w[i]), int(h[i])) for i in r}) == 1 for r in runs)
            assert len({(int(w[r[0]]), int(h[r[0]])) for r in runs}) == len(runs)
        off, total = lay_out(nbytes)
        padded = (nbytes + 15) // 16 * 16
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.uint64)[:n]) and total == int(padded.sum())


def test_no_follow_up_decoder_takes_what_its_base_did_not_leave(K):
    """The condition under which formats.files_offered changes no result at the refine seams: a follow-up decoder's probe
    takes (status 0) no file its base's probe gives a status other than 1 -- over every file of the tiff / tiffc / webp /
    webpl / webpa case modules, valid, refused and damaged, with the library's own ``ke_<kind>_probe`` (host code).  A decode
    only ever turns a 0 into a 2, so what holds for the probes holds for the calls.  And the helper itself: a base kind is
    offered every candidate, a follow-up its base's status-1 files among them, nothing where the base did not run."""
    import _tiff_cases as T
    import _tiffc_cases as TC
    import _webp_cases as W
    import _webpa_cases as WA
    import _webpl_cases as WL
    from kobato_eyes_amd.formats import files_offered

    lib = K._native.load_library()

    def files(*sets):
        return [next(x for x in (item if isinstance(item, tuple) else (item,)) if isinstance(x, bytes)) for s in sets for item in s]

    def probe(kind, blobs):
        sizes = np.array([len(b) for b in blobs], np.uint64)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
        flat = np.frombuffer(b"".join(blobs) + bytes(64), np.uint8)
        w, h, c, st = (np.zeros(len(blobs), np.int32) for _ in range(4))
        assert getattr(lib, f"ke_{kind}_probe")(flat.ctypes.data, offsets.ctypes.data, sizes.ctypes.data, len(blobs), w.ctypes.data,
                                                h.ctypes.data, c.ctypes.data, st.ctypes.data) == 0
        return st

    rng = np.random.default_rng(5)
    tif = files(T.supported(True), T.handmade(True), T.refused(), TC.valid_cases(), TC.refused_cases(), TC.late_change_cases(),
                TC.damaged_set(60))
    webp = files(W.taken_cases(), W.refused_cases(), WL.taken_cases(), WL.refused_cases(), WA.all_taken(), WA.refused_cases())
    for base in files(W.taken_cases()[:12], WL.fuzz_bases(), WA.fuzz_bases()):
        webp += files(W.damaged(base, rng, 20), WA.damaged(base, rng, 20))
    for base, follow_up, blobs in (("tiff", "tiffc", tif), ("webp", "webpl", webp), ("webp", "webpa", webp)):
        st, st2 = probe(base, blobs), probe(follow_up, blobs)
        assert (st == 0).any() and (st == 1).any() and (st == 2).any() and (st2 == 0).any()       # the sets reach every answer
        assert not ((st != 1) & (st2 == 0)).any(), (base, follow_up, np.nonzero((st != 1) & (st2 == 0))[0][:10].tolist())
    ran = {"webp": (["a", "b", "c", "d"], [0, 1, 2, 1])}
    assert files_offered("webp", ["d", "b", "x"], {}) == ["d", "b", "x"] and files_offered("jpeg", [], ran) == []
    assert files_offered("webpl", ["x", "d", "c", "b", "a"], ran) == ["d", "b"] and files_offered("webpa", ["b"], ran) == ["b"]
    assert files_offered("tiffc", ["a", "b"], ran) == [] and files_offered("webpl", ["a", "b"], {}) == []


def test_bench_self_launches_its_ranks_world_size_2_gloo():
    """`python bench.py --gpus 2` typed without a launcher (as the driver types it at N = 1) must start its ranks as fresh
    child processes under torch.distributed.run, relay rank 0's one JSON line on stdout and return the children's exit
    code.  Without a GPU the ranks only meet (gloo) and count each other."""
    import json

    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--rendezvous-only"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["n_ranks_seen"] == 2 and out["world_size"] == 2 and out["self_launched"] is True
    # a failing rank is the launcher's failure too
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rendezvous-only", "--no-such-flag"],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0
