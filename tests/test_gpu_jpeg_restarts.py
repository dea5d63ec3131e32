"""Restart intervals on separate lanes (KE_JPEG_SPLIT_RESTARTS=1; csrc/ke_jpeg_restarts.h, ke_jpeg_find_restarts and
ke_jpeg_entropy_rst in csrc/ke_jpeg.hip): the statuses and every byte of every taken file are those of the one-lane walk --
the variable unset -- and Pillow's; ke_jpeg_last_split shows that the lanes really ran, for exactly the files the rule admits;
files the rule declines, damaged files, the scaled decode and the batch hasher's seam give what they give without it.

All files are tiny (tests/_jpeg_rst_cases.py); KE_JPEG_SPLIT_MIN_MCUS=1 makes lanes of single intervals in them, the default
of 64 leaves two of them split."""
from __future__ import annotations

import faulthandler
import functools
import os

import numpy as np
import pytest

import _jpeg_cases as C
import _jpeg_rst_cases as R
import _jpeg_stream_cases as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SPLIT, MIN_MCUS = "KE_JPEG_SPLIT_RESTARTS", "KE_JPEG_SPLIT_MIN_MCUS"


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


class _env:
    """The two variables for the length of a block: split on or off, the minimum of MCUs per lane or the default."""

    def __init__(self, split: bool, min_mcus=None):
        self.want = {SPLIT: "1" if split else None, MIN_MCUS: None if min_mcus is None else str(min_mcus)}

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.want}
        for k, v in self.want.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _decode(ctx, blobs, split, min_mcus=None):
    """-> (pixels, statuses, (files split, lanes))"""
    with _env(split, min_mcus), time_limit(60):
        out, status = ctx.jpeg_decode(list(blobs))
        return out, [int(s) for s in status], ctx.jpeg_last_split()


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b))


def _assert_alike(names, unset, other):
    wrong = [(names[k], unset[1][k], other[1][k]) for k in range(len(names)) if unset[1][k] != other[1][k] or not _same(unset[0][k], other[0][k])]
    assert not wrong, wrong[:20]


@functools.lru_cache(maxsize=None)
def _big_batch():
    """[(name, file, Pillow's pixels or None)], shuffled: restart files of every make, and files the path must leave alone."""
    cases = [(name, data, S.pillow(data)) for name, data, _ in S.family("restarts")]                   # sequential and progressive
    cases += [(name, data, ref) for name, data, ref in C.supported() if name.startswith("restart_")]
    cases += [(name, data, S.pillow(data)) for name, data in R.handwritten()]
    cases += [(name, data, S.pillow(data)) for name, data, _ in S.family("stuffing")[:6]]             # no DRI
    cases += [(name, data, None) for name, data in S.refused()[:1]]
    order = np.random.default_rng(91).permutation(len(cases))
    return tuple(cases[k] for k in order)


@pytest.fixture(scope="module")
def big(ctx):
    """The batch decoded once with the variable unset, once with lanes of one interval, once with the default minimum."""
    blobs = [c[1] for c in _big_batch()]
    return {"unset": _decode(ctx, blobs, False), "min1": _decode(ctx, blobs, True, 1), "default": _decode(ctx, blobs, True)}


def test_split_files_decode_as_the_walk_does_and_as_pillow_does(big):
    cases = _big_batch()
    names = [c[0] for c in cases]
    for setting in ("min1", "default"):
        _assert_alike(names, big["unset"], big[setting])
        out, status, _ = big[setting]
        for k, (name, _, ref) in enumerate(cases):
            if name.startswith("refused_"):
                assert status[k] == 2 and out[k] is None, name
            else:
                assert status[k] == 0 and ref is not None and _same(out[k], ref), (setting, name)
    # the batch holds what it is there for
    seq = [c for c in cases if not c[0].startswith("refused_") and not R.header(c[1])[2]]
    assert sum(R.header(c[1])[2] for c in cases if not c[0].startswith("refused_")) >= 20                # progressive files
    assert sum(R.header(c[1])[1] == 0 for c in seq) >= 6                                                  # no DRI (or DRI 0)
    assert R.lanes_of(dict(R.handwritten())["rst_gray_140_intervals_of_1"], 1) == 140                    # more lanes than a wave
    assert max(R.lanes_of(c[1], 1) for c in seq) >= 140 and sum(R.lanes_of(c[1], 1) >= 2 for c in seq) >= 50


def test_the_split_really_ran(big):
    """ke_jpeg_last_split: files and lanes as the plan's definition gives them (every sequential file of this batch with a DRI
    is a valid one: the rule admits it whenever its plan has two lanes or more); zeros with the variable unset."""
    cases = _big_batch()
    valid = [c[1] for c in cases if not c[0].startswith("refused_")]
    assert big["unset"][2] == (0, 0)
    for setting, min_mcus in (("min1", 1), ("default", R.DEFAULT_MIN_MCUS)):
        lanes = [R.lanes_of(d, min_mcus) for d in valid]
        assert big[setting][2] == (sum(n >= 2 for n in lanes), sum(lanes)), setting
    assert big["default"][2][0] >= 2 and big["min1"][2][1] >= 140


def test_declined_files_keep_their_verdict(ctx):
    """Each deviant in a batch of good files: the status and the pixels of the walk, the status named in the case where there is
    one, and ke_jpeg_last_split counts the files the rule admits and no other."""
    good = list(R.handwritten()[:12])
    for name, data, verdict, expected in R.deviants():
        names = [g[0] for g in good[:6]] + [name] + [g[0] for g in good[6:]]
        blobs = [g[1] for g in good[:6]] + [data] + [g[1] for g in good[6:]]
        unset, split = _decode(ctx, blobs, False), _decode(ctx, blobs, True, 1)
        _assert_alike(names, unset, split)
        assert unset[2] == (0, 0)
        if expected is not None:
            assert split[1][6] == expected, name
        if split[1][6] == 0:
            assert _same(split[0][6], S.pillow(data)), name
        admitted = [g[1] for g in good] + ([data] if verdict == "split" else [])
        lanes = [R.lanes_of(d, 1) for d in admitted]
        assert split[2] == (sum(n >= 2 for n in lanes), sum(lanes)), name
    assert {v for _, _, v, _ in R.deviants()} == {"numbers", "few", "refused", "many", "split"}


def _scan_range(data: bytes):
    at = data.index(b"\xff\xda")
    return at + 2 + int.from_bytes(data[at + 2:at + 4], "big"), len(data) - 2


def test_damaged_files_decode_alike(ctx):
    """12 restart files, each with 30 single bytes of its entropy data changed and 10 changes to its DRI payload, in one call:
    set and unset agree on every status and on every taken file's bytes."""
    picked = [c for c in R.handwritten() if R.lanes_of(c[1], 1) >= 3]
    picked = picked[::max(1, len(picked) // 12)][:12]
    assert len(picked) == 12
    rng = np.random.default_rng(92)
    names, blobs = [], []
    for name, data in picked:
        lo, hi = _scan_range(data)
        dri = R.header(data)[3]
        for k in range(30):
            b = bytearray(data)
            at = int(rng.integers(lo, hi))
            b[at] = (b[at] + int(rng.integers(1, 256))) & 255
            names.append(f"{name}_byte{k}@{at}")
            blobs.append(bytes(b))
        for k in range(10):
            b = bytearray(data)
            at = dri + (k & 1)
            b[at] = (b[at] + int(rng.integers(1, 256))) & 255
            names.append(f"{name}_dri{k}")
            blobs.append(bytes(b))
    unset, split = _decode(ctx, blobs, False), _decode(ctx, blobs, True, 1)
    _assert_alike(names, unset, split)
    assert unset[2] == (0, 0) and split[2][0] >= 100          # a change inside an interval leaves the markers as they are
    assert len(set(unset[1])) >= 2                            # some are still taken, some are not


def test_scaled_decode(ctx):
    """ke_jpeg_decode_scaled at 1/2 and 1/8: the same path in front of the reduced transforms."""
    by_name = dict(R.handwritten())
    names = ["rst_420_17_intervals_of_2", "rst_gray_140_intervals_of_1", "rst_422_77x22_ri2_ones"]
    blobs = [by_name[n] for n in names]
    for denom in (2, 8):
        results = {}
        for split in (False, True):
            with _env(split, 1), time_limit(60):
                out, status, used = ctx.jpeg_decode_scaled(blobs, denoms=[denom] * len(blobs))
                results[split] = (out, [int(s) for s in status], ctx.jpeg_last_split())
            assert list(used) == [denom] * len(blobs)
        _assert_alike(names, results[False], results[True])
        assert results[False][1] == [0, 0, 0] and results[False][2] == (0, 0)
        lanes = [R.lanes_of(b, 1) for b in blobs]
        assert results[True][2] == (3, sum(lanes)) and min(lanes) >= 2


def test_batch_hasher_rows(ctx, tmp_path):
    """fast_fill_missing_signatures over 32 restart files on disk: the rows with the variable set are the rows without it, and
    the hashes of Pillow's pixels."""
    import kobato_eyes_amd as K

    items, expected = [], {}
    rng = np.random.default_rng(93)
    for k in range(32):
        w, h = int(rng.integers(40, 120)), int(rng.integers(40, 120))
        arr = O.synth_rgb(300 + k, w, h)
        path = tmp_path / f"rst_{k:02d}.jpg"
        C.Image.fromarray(arr).save(path, "JPEG", quality=85, subsampling=(0, 1, 2)[k % 3], **({"restart_marker_rows": 1} if k % 2 else {"restart_marker_blocks": 3}))
        items.append((k + 1, str(path)))
        ep, ed = O.hash_image(np.asarray(C.Image.open(path)))
        expected[k + 1] = (O.to_signed64(ep), O.to_signed64(ed))
    fill = lambda: K.fast_fill_missing_signatures("", items, max_workers=2, chunksize=16, apply_to_db=False)      # noqa: E731
    with _env(True, 1), time_limit(120):
        rows_set = fill()
        split = ctx.jpeg_last_split()
    with _env(False), time_limit(120):
        rows_unset = fill()
        assert ctx.jpeg_last_split() == (0, 0)
    assert rows_set == rows_unset and [(fid, expected[fid][0], expected[fid][1]) for fid, _ in items] == [tuple(r) for r in rows_set]
    lanes = [R.lanes_of(open(p, "rb").read(), 1) for _, p in items]
    assert split == (32, sum(lanes)) and min(lanes) >= 2
