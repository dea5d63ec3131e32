"""Files for the tests of the restart-interval split (KE_JPEG_SPLIT_RESTARTS; csrc/ke_jpeg_restarts.h): sequential files with
restart intervals written coefficient by coefficient (tests/_jpeg_write.py) -- every sampling, intervals of 1, 2, 3, 7, of all
MCUs but one, of all and of one more, of 65 535, 9 / 10 / 17 intervals (the RSTn numbering wraps at 8), 140 intervals of one
MCU (more lanes than a wave), both kinds of padding, a stuffed FF 00 as the last data byte in front of a marker -- and the
deviants the rule must hand to the one-lane walk.  Also the plan and the header facts restated in Python, from the plan's
definition, for the tests to compute what they expect."""
from __future__ import annotations

import functools
import struct

import numpy as np

import _jpeg_stream_cases as S
import _jpeg_write as W

LANE_CAP = 16384
DEFAULT_MIN_MCUS = 64


def plan(mcus: int, ri: int, min_mcus: int = DEFAULT_MIN_MCUS, cap: int = LANE_CAP):
    """(intervals, intervals per lane, lanes): g is the smallest count that gives a lane at least min_mcus MCUs (or the whole
    file) and keeps the lanes at or below cap -- by search, not by the header's closed form."""
    if ri == 0:
        return 1, 1, 1
    n_int = -(-mcus // ri)
    for g in range(1, n_int + 1):
        if (g * ri >= min_mcus or g == n_int) and -(-n_int // g) <= cap:
            return n_int, g, -(-n_int // g)
    raise AssertionError((mcus, ri, min_mcus, cap))


def header(data: bytes):
    """(MCUs, restart interval, progressive, offset of the DRI payload or None) from the segments in front of the first scan."""
    pos, ri, dri_at, frame = 2, 0, None, None
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF, pos
        marker, length = data[pos + 1], struct.unpack(">H", data[pos + 2:pos + 4])[0]
        if marker in (0xC0, 0xC1, 0xC2):
            h, w, n = struct.unpack(">HHB", data[pos + 5:pos + 10])
            hs, vs = (data[pos + 11] >> 4, data[pos + 11] & 15) if n > 1 else (1, 1)
            frame = (-(-w // (8 * hs))) * (-(-h // (8 * vs))), marker == 0xC2
        elif marker == 0xDD:
            ri, dri_at = struct.unpack(">H", data[pos + 4:pos + 6])[0], pos + 4
        elif marker == 0xDA:
            return frame[0], ri, frame[1], dri_at
        pos += 2 + length
    raise AssertionError("no scan")


def lanes_of(data: bytes, min_mcus: int = DEFAULT_MIN_MCUS) -> int:
    """Lanes the split gives a VALID file: 0 where it stays on the walk (progressive, no DRI, a plan of one lane)."""
    mcus, ri, progressive, _ = header(data)
    if progressive or ri == 0:
        return 0
    n_lanes = plan(mcus, ri, min_mcus)[2]
    return n_lanes if n_lanes >= 2 else 0


def _write(seed, sampling, w, h, ri, **kw):
    comps = S.components(sampling)
    coefs = S.coefficients(np.random.default_rng([31, seed]), w, h, comps)
    return W.write(w, h, comps, coefs, S.steps(2, 3), S.shaper("random2", "random2", 800 + seed), restart=ri, **kw)


def _size(sampling, mcus_x, mcus_y):
    hs, vs = S.FACTORS[sampling] or (1, 1)
    return mcus_x * 8 * hs - 3, mcus_y * 8 * vs - 2           # not whole MCUs


@functools.lru_cache(maxsize=None)
def handwritten():
    """[(name, file)]: all valid; Pillow opens every one."""
    cases, seed = [], 0
    for sampling in ("gray", "444", "422", "420", "440"):
        w, h = _size(sampling, 5, 3)                              # 15 MCUs
        for ri in (1, 2, 3, 7, 14, 15, 16, 65535):
            data, facts = _write(seed, sampling, w, h, ri, pad_ones=bool(seed % 2))
            assert len(facts.restarts) == (-(-15 // ri) - 1 if ri <= 15 else 0)
            cases.append((f"rst_{sampling}_{w}x{h}_ri{ri}_{'ones' if seed % 2 else 'zeros'}", data))
            seed += 1
    for n in (9, 10, 17):                                         # RST0 .. RST7, RST0, ...
        for ones in (True, False):
            data, facts = _write(seed, "gray", 8 * n - 1, 7, 1, pad_ones=ones)
            assert len(facts.restarts) == n - 1
            cases.append((f"rst_gray_{n}_intervals_{'ones' if ones else 'zeros'}", data))
            seed += 1
    data, facts = _write(seed, "420", 17 * 16, 32, 2)
    assert len(facts.restarts) == 16
    cases.append(("rst_420_17_intervals_of_2", data))
    seed += 1
    data, facts = _write(seed, "gray", 8, 1120, 1)               # more lanes than a wave from one file
    assert len(facts.restarts) == 139
    cases.append(("rst_gray_140_intervals_of_1", data))
    seed += 1
    data, facts = _write(seed, "gray", 16, 1120, 7, pad_ones=False)     # 280 MCUs, 40 intervals: 4 lanes at the default minimum
    assert len(facts.restarts) == 39
    cases.append(("rst_gray_16x1120_ri7", data))
    seed += 1
    for tries in range(400):                                      # a stuffed FF 00 as the last data byte in front of a marker
        data, facts = _write(1000 + tries, "gray", 8 * 12, 8, 1, pad_ones=True)
        if any(p - 2 in facts.stuffed for p in facts.restarts):
            cases.append(("rst_gray_stuffed_pair_in_front_of_a_marker", data))
            break
    else:
        raise AssertionError("no stuffed pair in front of a marker")
    assert len({name for name, _ in cases}) == len(cases)
    return tuple(cases)


def _cut(data: bytes, facts, ordinal: int, count: int) -> bytes:
    """`count` bytes taken out right in front of restart marker `ordinal` (none of them part of a stuffed pair)."""
    at = facts.restarts[ordinal]
    assert at - count >= (facts.restarts[ordinal - 1] + 2 if ordinal else facts.scan_offsets[0])
    assert 0xFF not in data[at - count - 1:at]
    return data[:at - count] + data[at:]


@functools.lru_cache(maxsize=None)
def deviants():
    """[(name, file, verdict of ke_rst_index with one-MCU lanes -- split / numbers / few / many / refused (by the parser) --,
    status the decoder must give or None where only 'as with the variable unset' is asked)]."""
    cases = []
    w, h = 61, 30                                                 # gray: 8 x 4 = 32 MCUs
    data, _ = _write(50, "gray", w, h, 3, rst_number=lambda k: k + (k >= 2))
    cases.append(("dev_wrong_number_on_marker_2", data, "numbers", 2))
    data, _ = _write(51, "gray", w, h, 5, stop_after=13)
    cases.append(("dev_data_stops_early", data, "few", 2))
    data, _ = _write(52, "gray", w, h, 4, before_marker={1: b"\xff"})
    cases.append(("dev_fill_bytes_in_front_of_a_marker", data, "refused", 1))
    data, facts = _write(53, "gray", w, h, 4)
    assert len(facts.restarts) == 7
    data, _ = _write(53, "gray", w, h, 4, before_marker={"eoi": bytes([0xFF, 0xD0 + 7])})
    cases.append(("dev_extra_rst_behind_the_last_interval", data, "many", None))
    data, _ = _write(54, "gray", w, h, 4, before_marker={1: b"\x00\x12\x34", 5: b"\x55"})
    cases.append(("dev_leftover_bytes_in_front_of_markers", data, "split", 0))
    # 4:2:0, 6 x 3 MCUs, an interval of 3: the last MCU of the second interval is not there (6 blocks: more bits than any padding)
    w2, h2 = _size("420", 6, 3)
    missing = {(0, r, c): [] for r in (0, 1) for c in (10, 11)}
    missing.update({(1, 0, 5): [], (2, 0, 5): []})
    data, facts = _write(55, "420", w2, h2, 3, override=missing)
    assert len(facts.restarts) == 5
    cases.append(("dev_interval_one_mcu_short", data, "split", 2))
    data, facts = _write(56, "gray", w, h, 4)
    for ordinal in range(1, 7):
        try:
            cases.append(("dev_interval_cut_runs_dry", _cut(data, facts, ordinal, 3), "split", None))
            break
        except AssertionError:
            continue
    else:
        raise AssertionError("no interval to cut")
    return tuple(cases)
