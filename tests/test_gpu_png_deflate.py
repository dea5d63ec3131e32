"""The GPU PNG inflate (csrc/ke_png.hip: the copy records, matches held back, the 64-byte stream ring; csrc/ke_lz_copies.h: runs,
phases, blockers inside a group of 64) on hand-written deflate streams (tests/_deflate_write.py, tests/_png_cases.py): the
valid, the invalid and the random set in ONE call, shuffled, so that the 64 lanes of a wave hold unlike streams and refusals
sit beside good files.  The judge is Pillow; the host build of the same header must agree on every status."""
from __future__ import annotations

import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _png_cases as P
import test_png_cpu as T
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_state = {"device_suspect": None}      # set when a step ended on a signal or a time limit: nothing more is started on the card


class time_limit:
    """A time limit of its own around one GPU step, sized to it: a call that hangs in native code ends the whole run (a Python
    exception could not interrupt it), so nothing more is started on the device."""

    def __init__(self, seconds: int) -> None:
        self.seconds = seconds

    def __enter__(self):
        if _state["device_suspect"]:
            pytest.fail(f"not started: {_state['device_suspect']}")
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    from kobato_eyes_amd import _native

    with time_limit(60):
        return _native.get_context(0)


@pytest.fixture(scope="module")
def batch(ctx):
    """(cases, pixels, statuses) of all three sets decoded in one call, in a shuffled order (fixed seed), put back in order."""
    cases = list(T.valid_cases()) + list(T.invalid_cases()) + list(T.random_cases())
    order = np.random.default_rng(64).permutation(len(cases))
    with time_limit(90):                                              # about 1 600 small files: seconds
        out, status = ctx.png_decode([cases[k][1] for k in order])
    pixels, statuses = [None] * len(cases), [None] * len(cases)
    for at, k in enumerate(order):
        pixels[k], statuses[k] = out[at], int(status[at])
    return cases, pixels, statuses


def test_one_shuffled_batch_decodes_as_pillow_does_and_as_the_host_build(batch):
    cases, pixels, statuses = batch
    nv, ni = len(T.valid_cases()), len(T.invalid_cases())
    answers = {id(c[1]): (statuses[k], pixels[k]) for k, c in enumerate(cases)}
    decode = lambda data: answers[id(data)]
    failures = T.hold_to_pillow(cases[:nv], decode, exact=True) + T.hold_to_pillow(cases[nv:nv + ni], decode, exact=False) + \
        T.hold_to_pillow(cases[nv + ni:], decode, exact=True)
    assert not failures, "\n".join(failures[:20])
    # the kernels and the host build compile the same header: a status that differs is a kernel bug
    L = T._lib()
    differ = [c[0] for k, c in enumerate(cases) if T._decode(L, c[1])[0] != statuses[k]]
    assert not differ, differ[:20]
    assert len(cases) == nv + ni + T.RANDOM_BLOCK_LISTS and nv >= 240 and ni >= 360


def test_single_file_calls_equal_the_batch(ctx, batch):
    """A file's result does not depend on the lanes beside it: 64 files, each in a call of its own."""
    cases, pixels, statuses = batch
    for k in np.random.default_rng(65).choice(len(cases), 64, replace=False):
        with time_limit(30):
            out, status = ctx.png_decode([cases[k][1]])
        assert int(status[0]) == statuses[k], cases[k][0]
        assert P.pixel_digest(out[0]) == P.pixel_digest(pixels[k]), cases[k][0]


def test_the_result_does_not_depend_on_how_many_matches_are_held_back(batch, tmp_path):
    """KE_PNG_HOLD = 1 (every match at once) and 64 (matches only when every stream waits) in fresh processes, one at a time,
    against the default in this process: same statuses, same pixels."""
    cases, pixels, statuses = batch
    nv, ni = len(T.valid_cases()), len(T.invalid_cases())
    keep = list(range(nv)) + list(range(nv + ni, len(cases)))
    worker = os.path.join(ROOT, "tests", "_png_hold_worker.py")
    for hold in ("1", "64"):
        path = str(tmp_path / f"hold{hold}.json")
        if _state["device_suspect"]:
            pytest.fail(f"not started: {_state['device_suspect']}")
        try:                                                          # the child builds its cases first (most of its time)
            res = subprocess.run([sys.executable, worker, ROOT, path], env=dict(os.environ, KE_PNG_HOLD=hold), capture_output=True, text=True,
                                 timeout=300)
        except subprocess.TimeoutExpired:
            _state["device_suspect"] = f"the KE_PNG_HOLD={hold} child ran into its time limit"
            raise
        if res.returncode < 0 or res.returncode in (124, 134, 137, 139):
            _state["device_suspect"] = f"the KE_PNG_HOLD={hold} child ended with {res.returncode}"
        assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
        with open(path) as f:
            got = json.load(f)
        assert got["hold"] == hold and len(got["status"]) == len(keep)
        for at, k in enumerate(keep):
            assert got["status"][at] == statuses[k] == 0, (hold, cases[k][0])
            assert got["digest"][at] == P.pixel_digest(pixels[k]), (hold, cases[k][0])


def test_decode_and_hash_without_leaving_the_gpu(ctx):
    """png_hash on every case of at least 16 x 16 pixels against the oracle's hashes of Pillow's pixels: the random set's
    larger images and the three many-row images of the valid set (its other streams are one-row images)."""
    cases = [c for c in list(T.valid_cases()) + list(T.random_cases()) if min(c[2].shape[:2]) >= 16]
    assert sum(1 for c in cases if c[0].startswith("rows_")) == 3
    with time_limit(60):
        ph, dh, st = ctx.png_hash([c[1] for c in cases])
    for k, c in enumerate(cases):
        assert st[k] == 0 and (int(ph[k]), int(dh[k])) == O.hash_image(c[2]), c[0]
    assert len(cases) >= 200
