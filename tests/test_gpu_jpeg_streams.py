"""The GPU JPEG decoder (csrc/ke_jpeg.hip) on hand-written entropy streams (tests/_jpeg_write.py, tests/_jpeg_stream_cases.py):
what only exists on the device -- the lane's 64-byte stream window with its 4-byte fast path (bits_fill / stream_dword), the
progressive kernel's own canonical tables (prog_build / ProgReader::sym), the choice between Huffman tables in LDS and in
global memory, the search for the end of the data (ke_jpeg_find_end) -- on Huffman tables of chosen shapes, stuffed pairs, the
end of the data and restart markers at chosen offsets, and end-of-band runs of every size.  The judge is Pillow; the host
build of the same headers (tests/test_jpeg_cpu.py) must agree on every status."""
from __future__ import annotations

import faulthandler
import functools

import numpy as np
import pytest

import _jpeg_stream_cases as S
import _jpeg_write as W
import test_jpeg_cpu as T
from oracle import oracle as O

pytestmark = pytest.mark.gpu


class time_limit:
    """A call that hangs in native code ends the whole run (a Python exception could not interrupt it)."""

    def __init__(self, seconds: int) -> None:
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    from kobato_eyes_amd import _native

    with time_limit(60):
        return _native.get_context(0)


def _equal(out, ref):
    return out is not None and out.shape == ref.shape and np.array_equal(out, ref)


def test_one_shuffled_batch_decodes_as_pillow_does_and_as_the_host_build(ctx):
    """All valid, tolerated and refused cases in ONE call, shuffled: statuses equal the host build's file by file, every valid
    file is taken with Pillow's pixels, a tolerated file that is taken has Pillow's pixels."""
    valid, tolerated, refused = S.valid(), S.tolerated(), S.refused()
    names = [c[0] for c in valid + tolerated + refused]
    blobs = [c[1] for c in valid + tolerated + refused]
    order = np.random.default_rng(71).permutation(len(blobs))
    with time_limit(60):
        out, status = ctx.jpeg_decode([blobs[k] for k in order])
    pixels, statuses = [None] * len(blobs), [None] * len(blobs)
    for at, k in enumerate(order):
        pixels[k], statuses[k] = out[at], int(status[at])
    refs = S.references()
    L = T._lib()
    wrong = [(names[k], statuses[k]) for k in range(len(blobs)) if statuses[k] != T._decode(L, blobs[k])[0]]
    assert not wrong, wrong[:20]
    wrong = [(names[k], statuses[k]) for k in range(len(valid)) if statuses[k] != 0 or not _equal(pixels[k], refs[names[k]])]
    assert not wrong, wrong[:20]
    for k, (name, _, expected, _) in enumerate(tolerated, len(valid)):
        assert statuses[k] == expected, name
        assert _equal(pixels[k], refs[name]) if expected == 0 else pixels[k] is None, name
    for k, (name, _) in enumerate(refused, len(valid) + len(tolerated)):
        assert statuses[k] == 2 and pixels[k] is None, name
    assert len(valid) >= 300 and len(tolerated) == 13 and len(refused) == 5


@functools.lru_cache(maxsize=None)
def _table_path_files(gray: bool, own_tables: bool, table_seed: int = 0):
    """32 coefficient sets as sequential files: with one set of hand-built tables for all of them (2 for gray files, 4 for colour
    files: at most kLdsTables a workgroup, whoever shares it), or each with tables of its own under ids of its own (2 a gray
    file, 6 a colour file: more than kLdsTables in any workgroup of three files or of one; table_seed: another set of them)."""
    files = []
    shared_rng = np.random.default_rng(72)
    shared = {(0, 0): W.random(shared_rng, list(range(12)), 2, True), (1, 0): W.random(shared_rng, list(range(256)), 4),
              (0, 1): W.ladder(list(range(11, -1, -1)), 5, True), (1, 1): W.full_256([0x00, 0xF0, 0x11, 0x01])}
    for k in range(32):
        rng = np.random.default_rng([73, k])
        w, h = int(rng.integers(9, 65)), int(rng.integers(9, 49))
        sampling = "gray" if gray else ("444", "422", "420", "440")[k % 4]
        ids = (0, 1, 1) if not own_tables else ((0, 1, 2), (1, 2, 3), (3, 0, 1))[k % 3]
        comps = S.components(sampling, td=ids, ta=ids[::-1] if own_tables else ids)
        coefs = S.coefficients(rng, w, h, comps)
        tabs = S.shaper(("random2", "ladder5", "edge", "inverted")[k % 4], ("random3", "all16", "inverted", "edge")[k % 4], 900 + k + 1000 * table_seed) if own_tables else shared
        data, facts = W.write(w, h, comps, coefs, S.steps(2, 3), tabs, restart=(0, 0, 3)[k % 3])
        assert len({t.payload for t in facts.tables.values()}) == ((2 if gray else 6) if own_tables else (2 if gray else 4))
        files.append(data)
    return tuple(files)


@pytest.mark.parametrize("gray", [True, False], ids=["gray", "colour"])
def test_tables_in_lds_and_tables_in_global_memory_decode_alike(ctx, gray):
    """ke_jpeg_entropy keeps at most four distinct tables of a workgroup in LDS and reads them from global memory otherwise: one
    call whose files all carry the same 2 (gray) or exactly 4 (colour) tables, one whose files carry 2 or 6 of their own.  The
    same coefficient sets both ways: the pixels are each other's and Pillow's.  (32 files are parsed by one host thread: the
    merge of several threads' table pools is the next test's.)"""
    lds, glob = _table_path_files(gray, False), _table_path_files(gray, True)
    with time_limit(60):
        out_lds, st_lds = ctx.jpeg_decode(lds)
        out_glob, st_glob = ctx.jpeg_decode(glob)
    for k in range(len(lds)):
        ref = S.pillow(lds[k])
        assert ref is not None and _equal(S.pillow(glob[k]), ref), k
        assert st_lds[k] == 0 and st_glob[k] == 0, k
        assert _equal(out_lds[k], ref) and _equal(out_glob[k], ref), k


def test_table_pools_of_two_host_threads_are_merged_and_remapped(ctx, monkeypatch):
    """ke_jpeg_decode parses a call's headers on one host thread per 256 files, each with a table pool (and a scan list) of its
    own, interns every pool again into the call's and remaps the files' table indices (part_index, remaps, scan_base).  544
    files, shuffled, in two parts: the 32 coefficient sets 16 times over -- each time with tables of their own from fresh
    seeds, or with the four shared ones, which the second thread's pool holds at other indices than the merged pool does --
    and the progressive files of prog_tables_ among them, so that the second part's scans do not begin at 0."""
    files, refs = [], []
    base = {gray: [S.pillow(d) for d in _table_path_files(gray, False)] for gray in (True, False)}
    for rep in range(16):
        gray = rep % 4 == 3
        files += _table_path_files(gray, rep % 3 != 2, rep if rep % 3 != 2 else 0)
        refs += base[gray]
    prog = S.family("prog_tables")
    files += [c[1] for c in prog] + [c[1] for c in prog[:8]]
    refs += [S.references()[c[0]] for c in prog] + [S.references()[c[0]] for c in prog[:8]]
    order = np.random.default_rng(74).permutation(len(files))
    files, refs = [files[k] for k in order], [refs[k] for k in order]
    assert len(files) // 256 >= 2 and any(b"\xff\xc2" in f[:400] for f in files[:272]) and any(b"\xff\xc2" in f[:400] for f in files[272:])
    monkeypatch.setenv("KE_HOST_THREADS", "4")                     # two threads (256 files each at least) whatever the machine has
    with time_limit(60):
        out, status = ctx.jpeg_decode(files)
    wrong = [k for k in range(len(files)) if status[k] != 0 or not _equal(out[k], refs[k])]
    assert not wrong, wrong[:20]


def test_end_of_data_found_on_the_device_or_on_the_host(ctx, monkeypatch):
    """stuffing_, ends_ and restarts_ twice: with ke_jpeg_find_end deciding where the entropy data ends, and with the host's
    walk (KE_JPEG_HOST_END).  Statuses and pixels are the same both ways, and Pillow's."""
    cases = S.family("stuffing") + S.family("ends") + S.family("restarts")
    blobs = [c[1] for c in cases]
    refs = S.references()
    monkeypatch.delenv("KE_JPEG_HOST_END", raising=False)
    with time_limit(60):
        out_dev, st_dev = ctx.jpeg_decode(blobs)
    monkeypatch.setenv("KE_JPEG_HOST_END", "1")
    with time_limit(60):
        out_host, st_host = ctx.jpeg_decode(blobs)
    for k, (name, _, _) in enumerate(cases):
        assert st_dev[k] == 0 and st_host[k] == 0, name
        assert _equal(out_dev[k], refs[name]) and _equal(out_host[k], refs[name]), name
    assert len(cases) >= 200


def test_decode_and_hash_without_leaving_the_gpu(ctx):
    """jpeg_hash over the valid cases of at least 16 x 16 pixels against the oracle's hashes of Pillow's pixels."""
    refs = S.references()
    cases = [c for c in S.valid() if min(refs[c[0]].shape[:2]) >= 16]
    with time_limit(60):
        ph, dh, status = ctx.jpeg_hash([c[1] for c in cases])
    for k, c in enumerate(cases):
        assert status[k] == 0, c[0]
        assert (int(ph[k]), int(dh[k])) == O.hash_image(refs[c[0]]), c[0]
    assert len(cases) >= 250


def test_runs_of_16384_and_32767_blocks_in_a_call_of_their_own(ctx):
    """The gray file of 1 456 x 1 456 (33 124 blocks, flat but for a few): EOB0 .. EOB14 in one scan, a run of 32 767 in another."""
    (name, data, facts), = [c for c in S.valid() if c[0] == S.BIG]
    assert 16384 in facts.eobruns and 32767 in facts.eobruns
    with time_limit(60):
        out, status = ctx.jpeg_decode([data])
    assert status[0] == 0 and _equal(out[0], S.references()[name])
