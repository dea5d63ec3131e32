"""Every row of the single-pass kernel table (csrc/ke_hash_select.h) is run and held to the oracle (run with -m gpu on an
MI355X).  The parity tests pick shapes at random and by habit; none of them guarantees that each of the 70 instantiations is
reached.  The widths come from tests/golden/hash_single_pass_candidates.json -- what the nested switches before the table gave
every shape -- and not from a second copy of the table."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hash_single_pass_candidates.json")


def rows_with_their_smallest_width():
    """(row, width, channels, both hashes) per row: the smallest width at which the row is the first one tried, one workgroup
    per image (no band plan) -- with both hashes asked for exactly when the row is a both-hashes row."""
    with open(FIXTURE) as f:
        golden = json.load(f)
    first = {}
    for key, runs in golden["sweep"].items():
        c, d, p, h, _ = key.split()
        if h != "h16" or p != "p0":
            continue
        for w0, w1, rows in runs:
            if not rows:
                continue
            name = golden["rows"][rows[0]]
            both = name.split(",")[3] == "1"
            if both == (d == "d1") and w0 < first.get(name, (1 << 30,))[0]:
                first[name] = (w0, int(c[1:]), both)
    assert sorted(first) == sorted(golden["rows"]) and len(first) == 70
    return [(name,) + first[name] for name in golden["rows"]]


def test_every_row_of_the_table_equals_the_oracle(monkeypatch):
    """n = 2 random images at the row's smallest width, h = 16 (the lowest accepted height, one 16-row tile of the wide family)
    and h = 48 (one and a half 32-row tiles of the narrow family), once with one workgroup per image and once in band mode."""
    from kobato_eyes_amd import _native

    ctx = _native.get_context(0)
    rng = np.random.default_rng(70)
    bad = []
    for name, w, c, both in rows_with_their_smallest_width():
        for h in (16, 48):
            px = rng.integers(0, 256, (2, h, w) if c == 1 else (2, h, w, c), dtype=np.uint8)
            want = [O.hash_image(px[j])[:2] for j in range(2)]
            for min_images in ("1", "1000000000"):
                monkeypatch.setenv("KE_FUSED_MIN_IMAGES", min_images)
                got_p, got_d = ctx.hash_uniform(px, 2, w, h, c, want_dhash=both)
                for j in range(2):
                    if int(got_p[j]) != want[j][0] or (both and int(got_d[j]) != want[j][1]):
                        bad.append((name, w, h, c, both, min_images, j))
    assert not bad, bad
