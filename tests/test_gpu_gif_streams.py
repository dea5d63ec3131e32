"""The GPU GIF decoder (csrc/ke_gif.hip: the code walk through the 16-byte window of csrc/ke_lz_window.h and the record sink of
csrc/ke_lz_records.h; csrc/ke_lz_copies.h at length bias 2: runs, phases, blockers inside a round of 64) on hand-written code
streams (tests/_gif_write.py, tests/_gif_stream_cases.py): the valid, the invalid and the random set in ONE call, shuffled, so
that the 64 lanes of a wave hold unlike streams and refusals sit beside good files.  The judge is Pillow; the host build of
the same headers must agree on every status."""
from __future__ import annotations

import faulthandler

import numpy as np
import pytest

import _gif_stream_cases as S
import test_gif_cpu as T
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FLAT = ("one_colour_strings_up_to_3001", "one_colour_chain")

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
    cases = T.all_streams()
    order = np.random.default_rng(66).permutation(len(cases))
    with time_limit(90):                                              # about 1 300 small files and one of 4.5 M pixels: seconds
        out, status = ctx.gif_decode([cases[k][1] for k in order])
    pixels, statuses = [None] * len(cases), [None] * len(cases)
    for at, k in enumerate(order):
        pixels[k], statuses[k] = out[at], int(status[at])
    return cases, pixels, statuses


def test_one_shuffled_batch_decodes_as_pillow_does_and_as_the_host_build(batch):
    cases, pixels, statuses = batch
    answers = {id(c[1]): (statuses[k], pixels[k]) for k, c in enumerate(cases)}
    failures = T.hold_to_pillow(cases, lambda data: answers[id(data)])
    assert not failures, "\n".join(failures[:20])
    # the kernels and the host build compile the same headers: a status that differs is a kernel bug
    L = T._lib()
    differ = [c[0] for k, c in enumerate(cases) if T._decode(L, c[1])[0] != statuses[k]]
    assert not differ, differ[:20]
    assert len(cases) == len(S.valid()) + len(S.invalid()) + S.RANDOM_STREAMS and len(S.valid()) >= 200 and len(S.invalid()) >= 60


def test_single_file_calls_equal_the_batch(ctx, batch):
    """A file's result does not depend on the lanes beside it: 32 files, each in a call of its own -- the runs at distances 7,
    15 and 16 across a round of 64, the last strings cut to one pixel, the long strings, and 24 drawn by a fixed seed."""
    cases, pixels, statuses = batch
    must = [k for k, c in enumerate(cases) if c[0] in ("run_d7_3_2_2_across_a_round", "run_d15_3_2_2_2_2_2_2_across_a_round", "run_d16_8_8_across_a_round",
                                                         "run_d16_2_2_2_2_2_2_2_2", "last_string_cut_to_1_from_2_8x8", "last_string_cut_to_1_from_4_17x3",
                                                         "one_colour_strings_up_to_3001", "one_colour_chain")]
    assert len(must) == 8
    rest = [k for k in np.random.default_rng(67).permutation(len(cases)) if k not in must][:24]
    for k in must + rest:
        with time_limit(30):
            out, status = ctx.gif_decode([cases[k][1]])
        assert int(status[0]) == statuses[k], cases[k][0]
        if statuses[k] == 0:
            assert np.array_equal(out[0], pixels[k]), cases[k][0]


def test_decode_and_hash_without_leaving_the_gpu(ctx):
    """gif_hash on every case of at least 16 x 16 pixels against the oracle's hashes of Pillow's luma -- but for the two frames
    of one colour, named here (FLAT; the first has a single other pixel): whether the hash bits of a flat tile agree is not
    the decoder's matter, and their pixels are held by the batch test."""
    cases = [c for c in list(S.valid()) + list(S.random_streams()) if min(c[2].shape[:2]) >= 16 and c[0] not in FLAT]
    assert sum(1 for c in S.valid() if c[0] in FLAT) == len(FLAT)
    with time_limit(60):
        ph, dh, st = ctx.gif_hash([c[1] for c in cases])
    for k, c in enumerate(cases):
        assert st[k] == 0 and (int(ph[k]), int(dh[k])) == O.hash_image(c[2]), c[0]
    assert len(cases) >= 300
