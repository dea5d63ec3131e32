"""Hand-written GIF code streams (tests/_gif_write.py) inside the container of tests/_gif_cases.gif: a valid set that holds
every feature of `valid_features()`, an invalid set with one rule per stream and the status it must get, and a random set
drawn from every code valid at each point.  A case is (name, file, Pillow's luma under LOAD_TRUNCATED_IMAGES = False or
None, census or expected status).  Plus the census of the copy records the product's own sink makes of a stream.

What LZW cannot do, and the sets therefore do not ask for (test_gif_cpu.test_what_lzw_cannot_record asserts it on every
stream).  An entry begins where an earlier CODE's string begins and is one longer than it, so a copy at distance d reads
from a code's start, and the copy behind it continues it only if that code was followed by a one-pixel code.  A copy is
followed by a copy inside a run, not by a one-pixel code -- so every copy of a run but its last reads from in front of the
run's head: all but the last begin fewer than d pixels behind the head, a run has at most d / 2 + 1 copies (9 at distance
16, not the 70 a round of 64 lanes would want: the round's boundary is crossed by placing the run's head at lane 63), its
phases are 2 .. d - 1, and 0 for a last copy that reads the entry at the run's own head, never 1; no run has distance 1.
A string is at most one longer than the longest
string before it, so one of L pixels needs L (L + 1) / 2 pixels in front of it: 513 needs 131 841, 1 027 needs 528 378, 3 001
needs 4 504 501 -- one frame of the valid set, one colour, 2 125 x 2 125, holds them all; every other frame is at most
100 x 100.  A string longer than 16 at a distance of at most 16 is the KwKwK string of 17 alone."""
from __future__ import annotations

import functools
from collections import Counter

import numpy as np
from PIL import ImageFile

import _gif_cases as G
import _gif_write as W

PALETTE = np.repeat((255 - np.arange(256, dtype=np.uint8))[:, None], 3, 1)      # luma 255 - index: no two indices alike, not a gray ramp
CHUNKINGS = ((255,), (1,), (3, 17))


def strict_pillow(data: bytes):
    saved, ImageFile.LOAD_TRUNCATED_IMAGES = ImageFile.LOAD_TRUNCATED_IMAGES, False
    try:
        return G._pillow(data)
    except Exception:
        return None
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = saved


def comment(n: int) -> bytes:
    """A comment extension of n + 4 bytes in front of the descriptor (n in 1..255)."""
    return b"!\xfe" + bytes([n]) + b"c" * n + b"\x00"


def case(name, w, h, codes, bits=8, *, sizes=(255,), terminator=True, trailer=True, tail=b"", ext=b"", interlace=False, cut=None, marks=()):
    """tail: bytes behind the stream (in front of the trailer); cut: the file ends after that many bytes of the stream."""
    body, census = W.stream(codes, bits, sizes=sizes, terminator=terminator, want=w * h)
    if cut is not None:
        body, trailer = body[:cut], False
    data = G.gif(w, h, body + tail, palette=PALETTE, interlace=interlace, ext=ext, trailer=trailer)
    data_off = len(G.gif(w, h, b"", palette=PALETTE, interlace=interlace, ext=ext, trailer=False)) + 1
    census[f"data_off_mod_16_is_{data_off % 16}"] += 1
    census["interlaced_%dx%d" % (w, h)] += bool(interlace)
    for m in marks:
        census[m] += 1
    return name, data, strict_pillow(data), census


# ---- pieces of scripts ------------------------------------------------------------------------------------------------------------
def strings_up_to(s: W.Script, n: int, value=0):
    """A literal and KwKwK codes behind it: afterwards there is an entry of every length 2 .. n (one colour); -> {length: code}."""
    s.lit(value)
    first = s.r.next
    for _ in range(n - 1):
        s.kwkwk()
    s.lit(value + 1)
    return {k + 2: first + k for k in range(n - 1)}


def run(s: W.Script, d: int, lengths, *, pad_records=0):
    """Contiguous copies of the given lengths, all at distance d: their sources -- a code of length - 1, then a literal -- are
    written first (strings among them are copies themselves: the last one is the blocker right in front of the run), then
    literals up to d pixels, then "the entry d back" once per copy; where the copies span d pixels exactly, one more, which
    reads the entry at the run's own first copy (phase 0) -- behind a single copy that entry is the one being built.
    pad_records: that many two-pixel copies in front."""
    assert sum(lengths) <= d + 1 and min(lengths) >= 2
    have = strings_up_to(s, max(max(lengths) - 1, 2))
    for k in range(pad_records):
        s.lit(k + 2)
        s.kwkwk()
    s.lit(9)
    start = len(s.r.out)
    for k, n in enumerate(lengths):
        s.code(have[n - 1]) if n > 2 else s.lit(20 + k)
        if len(s.r.out) < start + d:
            s.lit(40 + k)
    while len(s.r.out) < start + d:
        s.lit(60 + len(s.r.out))
    for n in lengths:
        kind, _, length, dist = s.back(d)
        assert (kind, length, dist) == ("string", n, d), (kind, length, dist, n, d)
    if sum(lengths) == d:
        kind, _, length, dist = s.back(d) if len(lengths) > 1 else s.kwkwk()
        assert (length, dist) == (lengths[0] + 1, d), (kind, length, dist, d)
    return len(lengths) + (sum(lengths) == d)


def records_before_run(d, lengths):
    s = W.Script(8, 1 << 20)
    copies = run(s, d, lengths)
    return sum(1 for c in s.codes if c > s.r.end) - copies


def run_lengths(d):
    """Length lists for distance d >= 3: two-pixel copies (even phases), a three in front (odd phases), longer ones."""
    out = [[2] * ((d + 1) // 2), [d]]                            # [d]: one copy of d pixels and the entry being built behind it
    if d >= 4:
        out.append([3] + [2] * ((d - 2) // 2))
        out.append([d // 2, d - d // 2])
    if d >= 8:
        out.append([4, 3, 2])
    return out


def longest_run(d):
    """Copies in the longest run there is at distance d (see the module's docstring)."""
    return 2 if d < 4 else d // 2 + 1 if d % 2 == 0 else (d + 1) // 2


# ---- the valid set ----------------------------------------------------------------------------------------------------------------
def _valid():
    rng = np.random.default_rng(71)
    out = []

    def add(*a, **k):
        out.append(case(*a, **k))

    # widths and clear codes
    for bits in range(2, 9):
        w = h = 80
        s = W.Script(bits, w * h)
        s.lits_until(4096)
        for _ in range(520):                                     # the table stays full: literals, old entries, the newest one
            pick = int(rng.integers(0, 3))
            s.code(int(rng.integers(0, s.r.clear)) if pick == 0 else 4095 if pick == 1 else int(rng.integers(s.r.clear + 2, 4096)))
        s.fill()
        add(f"full_table_bits_{bits}", w, h, s.end().codes, bits)
    for name, at in (("in_mid_width", lambda wd: 3 << (wd - 2)), ("width_just_grown", lambda wd: 1 << (wd - 1)), ("one_code_before_growth", lambda wd: (1 << wd) - 1)):
        s = W.Script(2, 100 * 100)
        for wd in range(3, 13):
            target = max(at(wd), 7) if wd == 3 else at(wd)
            if target > 4096 or (name == "one_code_before_growth" and wd == 12):
                continue
            s.lits_until(target)
            assert s.r.width == wd, (name, wd, s.r.width, s.r.next)
            s.clear()
        s.fill()
        add(f"clear_{name}", 100, 100, s.end().codes, 2)
    s = W.Script(8, 64)
    s.lit(1, 2, 3)
    s.clear(2)
    s.lit(4, 5)
    s.clear(3)
    s.fill()
    s.clear()                                                    # behind the last pixel
    add("clears_in_a_row_and_behind_the_last_pixel", 8, 8, s.end().codes)
    s = W.Script(8, 64, open_clear=False)
    s.lit(5, 6, 5, 6)
    s.code(258)
    s.fill()
    add("no_opening_clear", 8, 8, s.end().codes)
    s = W.Script(8, 64)
    s.fill()
    add("no_end_code", 8, 8, s.codes)
    junk = b"\x03\xff\xff\xff\x01\x00\x02\x55\xaa\x00"
    add("junk_blocks_behind_the_end_code", 8, 8, s.codes + [s.r.end], terminator=False, tail=junk, marks=["junk_behind_the_end_code"])

    # KwKwK and strings
    s = W.Script(2, 72 * 72)
    s.lit(1)
    s.kwkwk()                                                    # the second code after a clear
    for wd in range(3, 13):
        s.lits_until(max(1 << (wd - 1), 7) if wd > 3 else 7)
        assert s.r.width == wd
        s.kwkwk()
    s.lits_until(4095)
    s.kwkwk()                                                    # code 4095 while the next free entry is 4095
    s.fill()
    add("kwkwk_at_every_width", 72, 72, s.end().codes, 2)
    s = W.Script(8, 80 * 80)
    s.lit(1, 2, 1, 2)                                            # "1 2" twice in the dictionary
    s.code(s.r.next - 1)                                         # the newest entry
    old = 258
    s.fill(keep=2)
    s.code(old)                                                  # made more than 4 000 pixels ago
    add("old_newest_and_duplicate_entries", 80, 80, s.end().codes)

    # piece lengths: one colour, every length 2 .. 3 001 as KwKwK, the listed ones again from their old entries
    w = h = 2125
    s = W.Script(8, w * h)
    have = strings_up_to(s, 3001, value=7)
    for n in W.LENGTHS + (3001,):
        s.lit(7) if s.r.out[-1] != 7 else None
        s.code(have[n])
    assert 513 < s.left() < 3001, s.left()
    s.code(have[3001])                                           # the last string, cut from above 513
    assert s.left() == 0
    add("one_colour_strings_up_to_3001", w, h, s.end().codes)
    s = W.Script(8, 100 * 100)                                   # each copy reads the one before it, 140 in a chain
    s.lit(3)
    while s.left() > 0:
        s.kwkwk()
    add("one_colour_chain", 100, 100, s.end().codes)

    # the last string
    for keep, n, name in ((3, 3, "ends_at_the_last_pixel"), (1, 2, "cut_to_1_from_2"), (1, 4, "cut_to_1_from_4"), (2, 3, "cut_to_2"), (2, 17, "cut_to_2_from_17")):
        for (w, h) in ((8, 8), (17, 3)):
            s = W.Script(8, w * h)
            have = strings_up_to(s, max(n, 2))
            s.fill(keep=keep)
            s.code(have[n])
            add(f"last_string_{name}_{w}x{h}", w, h, s.end().codes)
    s = W.Script(8, 64)
    s.lit(1)
    s.kwkwk()
    s.fill()
    add("last_code_a_literal", 8, 8, s.end().codes)
    s = W.Script(8, 64)
    s.lit(1, 2, 2)
    s.lit(4)
    s.kwkwk()                                                    # a lone copy at distance 1 between literals
    s.fill()
    add("lone_distance_1", 8, 8, s.end().codes)

    # runs: every distance 2..16, and 17 (contiguous, not a run); at the start of the records and across a round of 64
    s = W.Script(8, 64)
    s.lit(1, 2, 3)
    s.back(2)
    s.kwkwk()                                                    # distance 2: the entry 2 back, then the entry being built
    s.fill()
    add("run_d2", 8, 8, s.end().codes)
    for d in range(3, 18):
        for k, lengths in enumerate(run_lengths(d)):
            for across in (False, True):
                pad = (63 - records_before_run(d, lengths)) % 64 if across else 0
                w, h = (24, 24) if across else (16, 16)
                s = W.Script(8, w * h)
                run(s, d, lengths, pad_records=pad)
                s.fill()
                add(f"run_d{d}_{'_'.join(map(str, lengths))}{'_across_a_round' if across else ''}", w, h, s.end().codes, sizes=((255,), (1,), (16,))[(d + k) % 3])

    # sub-blocks and the window
    noise = rng.integers(0, 256, 64 * 64, dtype=np.uint8)
    greedy = W.encode(noise, 8)
    for sizes in ((1,), (2,), (15,), (16,), (17,), (254,), (255,), (15, 16, 17), (254, 255, 1), (1, 2, 15, 16, 17, 254, 255), (17, 1, 16, 2)):
        add(f"sub_blocks_{'_'.join(map(str, sizes))}", 64, 64, greedy, sizes=sizes)
    small = W.encode(noise[:400] & 15, 4, end=False)
    for n in range(1, 17):
        add(f"comment_of_{n}", 20, 20, small + [17], 4, ext=comment(n), sizes=(16, 5))
    for behind in range(0, 17):                                  # the last byte the decoder needs is the file's last, or 1..16 lie behind it
        add(f"ends_with_the_last_code_{behind}_behind", 20, 20, small, 4, terminator=False, trailer=False, tail=bytes(range(1, behind + 1)), sizes=(255,) if behind % 2 else (7,),
            marks=[f"bytes_behind_the_last_needed_one_{behind}"])

    # the writers' other choices, from given pixels
    periodic = np.tile(rng.integers(0, 8, 7, dtype=np.uint8), 200)[:32 * 32]
    add("pixels_no_opening_clear", 32, 32, W.encode(periodic, 3, open_clear=False), 3)
    add("pixels_clear_at_chosen_entries", 32, 32, W.encode(periodic, 3, clear_at=(15, 16, 31, 40)), 3)
    add("pixels_never_longer_than_3", 32, 32, W.encode(periodic, 3, max_len=3), 3, sizes=(2, 15))
    add("pixels_the_entry_7_back", 32, 32, W.encode(periodic, 3, d_back=7), 3)
    add("pixels_any_valid_code", 32, 32, W.encode(periodic, 3, rng=rng), 3, sizes=(17, 254))

    # interlace
    for w in (1, 3):
        for h in range(1, 18):
            a = rng.integers(0, 256, (h, w), dtype=np.uint8)
            add(f"interlaced_{w}x{h}", w, h, W.encode(G._rows_interlaced(a).ravel(), 8), interlace=True, sizes=(4,))
    return out


@functools.lru_cache(None)
def valid():
    return tuple(_valid())


def valid_features():
    f = [f"codes_with_a_full_table_bits_{b}" for b in range(2, 9)] + [f"clear_at_width_{w}" for w in range(3, 13)]
    f += ["clear_when_the_width_has_just_grown", "clear_one_code_before_the_width_grows", "clears_in_a_row_2", "clears_in_a_row_3", "clear_behind_the_last_pixel",
          "no_opening_clear", "end_code_behind_the_last_pixel", "no_end_code", "junk_behind_the_end_code", "no_block_terminator"]
    f += [f"kwkwk_at_width_{w}" for w in range(3, 13)] + ["kwkwk_second_code_after_a_clear", "kwkwk_at_next_4095", "code_equal_to_the_newest_entry",
                                                          "entry_used_4000_pixels_back", "duplicate_string_in_the_dictionary"]
    f += [f"length_{n}_{how}" for n in W.LENGTHS + ("above_3000",) for how in ("kwkwk", "old_entry")] + ["length_17_at_distance_16"]
    f += ["last_string_ends_at_the_last_pixel", "last_string_cut_to_1", "last_string_cut_to_2", "last_string_cut_from_above_513", "last_code_is_a_literal"]
    f += [f"sub_block_of_{n}" for n in (1, 2, 15, 16, 17, 254, 255)] + [f"data_off_mod_16_is_{k}" for k in range(16)]
    f += [f"size_byte_at_window_offset_{k}" for k in range(16)] + [f"code_split_after_{k}_bits" for k in range(1, 12)]
    f += [f"bytes_behind_the_last_needed_one_{k}" for k in range(17)] + [f"interlaced_{w}x{h}" for w in (1, 3) for h in range(1, 18)]
    return f


def record_features():
    """What the copy records of the valid set must hold (counted by records_census from the product's own records)."""
    f = [f"piece_of_{n}" for n in (2, 3, 15, 16, 17, 511, 512, 513)] + ["string_in_2_pieces", "string_in_3_pieces", "string_in_6_pieces", "last_piece_of_2_after_512",
                                                                       "record_into_the_slack"]
    for d in range(2, 17):
        f += [f"run_d{d}_of_{longest_run(d)}_copies"] + ([f"run_d{d}_continued_at_lane_0"] if d > 2 else [])
    f += [f"run_d{d}_phase_{p}" for d in (3, 7, 15, 16) for p in range(2, d)] + [f"run_d{d}_phase_0" for d in (3, 7, 15, 16)]
    f += ["run_of_2_pixel_copies", "run_of_longer_copies", "run_behind_a_blocker", "run_head_shorter_than_its_distance", "contiguous_copies_at_distance_17",
          "lone_copy_at_distance_1", "chain_of_100_dependent_copies_beyond_16"]
    return f


def records_census(rec: np.ndarray, want: int) -> Counter:
    """rec: n x 2 uint32 {destination, distance << 9 | (length - 2)}, as the sink wrote them."""
    c = Counter()
    n = len(rec)
    if n == 0:
        return c
    dst = rec[:, 0].astype(np.int64)
    dist = (rec[:, 1] >> 9).astype(np.int64)
    length = (rec[:, 1] & 511).astype(np.int64) + 2
    end = dst + length
    for v in np.unique(length):
        c[f"piece_of_{int(v)}"] += int((length == v).sum())
    c["record_into_the_slack"] += int((end > want).sum())
    c["lone_copy_at_distance_1"] += int(((dist == 1) & (length == 2)).sum())
    joined = np.zeros(n, bool)
    joined[1:] = (dst[1:] == end[:-1]) & (dist[1:] == dist[:-1])
    chain = best = 0
    k = 0
    while k < n:
        j = k
        while j + 1 < n and joined[j + 1]:
            j += 1
        copies, d = j - k + 1, int(dist[k])
        if copies > 1 and d > 16 and d >= 513:                    # the pieces of one long string
            c[f"string_in_{copies}_pieces"] += 1
            c["last_piece_of_2_after_512"] += int(length[j] == 2 and length[j - 1] == 512)
        elif copies > 1 and d == 17:
            c["contiguous_copies_at_distance_17"] += 1
        elif copies > 1 and d <= 16:
            c[f"run_d{d}_of_{copies}_copies"] += 1
            c["runs"] += 1
            c["runs_with_a_source_behind_the_head"] += int(dst[j - 1] - dst[k] >= d)      # all but the last copy read from in front of it
            c["run_of_2_pixel_copies"] += int((length[k:j + 1] == 2).all())
            c["run_of_longer_copies"] += int((length[k:j + 1] > 2).any())
            c["run_head_shorter_than_its_distance"] += int(length[k] < d)
            c["run_behind_a_blocker"] += int(k > 0 and end[k - 1] > dst[k] - d and dst[k - 1] < dst[k])
            for m in range(k + 1, j + 1):
                c[f"run_d{d}_phase_{int((dst[m] - dst[k]) % d)}"] += 1
                c[f"run_d{d}_continued_at_lane_0"] += int(m % 64 == 0)
        k = j + 1
    for k in range(1, n):                                        # copies that read what the one before them wrote, beyond 16
        src = dst[k] - dist[k]
        if dist[k] > 16 and src < end[k - 1] and src + min(dist[k], length[k]) > dst[k - 1]:
            chain += 1
            best = max(best, chain)
        else:
            chain = 0
    c["chain_of_100_dependent_copies_beyond_16"] += int(best >= 100)
    return c


# ---- the invalid set --------------------------------------------------------------------------------------------------------------
def _invalid():
    """(name, file, Pillow's luma or None, expected status): 2 = damaged (Pillow raises), 1 = left to Pillow."""
    out = []

    def add(name, w, h, codes, bits, status, **how):
        for sizes in CHUNKINGS:
            n, data, ref, _ = case(f"{name}_blocks_{'_'.join(map(str, sizes))}", w, h, codes, bits, sizes=sizes, **how)
            out.append((n, data, ref, status))

    def junk(s, n=40):
        return s.codes + [k % 4 for k in range(n)] + [s.r.end]

    for wd in range(3, 13):
        s = W.Script(2, 72 * 72)
        s.lits_until(max(1 << (wd - 1), 7) if wd > 3 else 6)
        assert s.r.width == wd and s.r.next + 1 < (1 << wd)
        s.codes.append(s.r.next + 1)
        add(f"code_beyond_next_at_width_{wd}", 72, 72, junk(s), 2, 2)
    for name, pre, code in (("first_code_is_next", (), 258), ("first_code_above_next", (), 300), ("first_code_after_a_clear_is_next", (1, 2, 3), 258),
                            ("first_code_after_a_clear_above_next", (1, 2, 3), 259)):
        s = W.Script(8, 64)
        if pre:
            s.lit(*pre)
            s.clear()
        s.codes.append(code)
        add(name, 8, 8, junk(s), 8, 2)
    for name, keep in (("at_the_first_code", 64), ("in_mid_stream", 30), ("one_pixel_short", 1)):
        s = W.Script(8, 64)
        s.fill(keep=keep)
        add(f"end_code_{name}", 8, 8, junk(s.end(), 10), 8, 1)
    s = W.Script(8, 64)
    s.fill(keep=9)
    add("block_terminator_before_the_last_pixel", 8, 8, s.codes, 8, 1)
    s = W.Script(8, 20 * 20)
    s.fill()
    for sizes in CHUNKINGS:
        body = W.stream(s.codes, 8, sizes=sizes, want=400)[0]
        ends, at = [], 1                                         # where the sub-blocks end
        while body[at]:
            at += 1 + body[at]
            ends.append(at)
        whole = ends[(len(ends) - 1) // 2]
        tag = "_".join(map(str, sizes))
        for name, cut in (("file_ends_at_a_size_byte", whole), ("file_ends_behind_a_size_byte", whole + 1), ("file_ends_inside_the_last_sub_block", len(body) - 2)):
            n, data, ref, _ = case(f"{name}_blocks_{tag}", 20, 20, s.codes, 8, sizes=sizes, cut=cut)
            out.append((n, data, ref, 2))
        if sizes[0] > 2:
            n, data, ref, _ = case(f"file_ends_inside_a_sub_block_blocks_{tag}", 20, 20, s.codes, 8, sizes=sizes, cut=whole + 2)
            out.append((n, data, ref, 2))
    return out


@functools.lru_cache(None)
def invalid():
    return tuple(_invalid())


# ---- the random set ---------------------------------------------------------------------------------------------------------------
RANDOM_STREAMS = 1000


def _random(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        bits, w, h = int(rng.integers(2, 9)), int(rng.integers(1, 41)), int(rng.integers(1, 41))
        s = W.Script(bits, w * h, open_clear=bool(rng.random() < 0.9))
        r = s.r
        while s.left() > 0:
            u = rng.random()
            if u < 0.02:
                s.clear()
            elif r.fresh or u < 0.45 or (u < 0.85 and r.next == r.clear + 2):
                s.code(int(rng.integers(0, r.clear)))
            elif u < 0.85 or r.next >= 4096:
                s.code(int(rng.integers(r.clear + 2, r.next)))
            else:
                s.kwkwk()
        if rng.random() < 0.5:
            s.end()
        sizes = tuple(int(v) for v in rng.integers(1, 256, int(rng.integers(1, 5))))
        if rng.random() < 0.5:
            sizes = tuple(int(v) for v in rng.choice([1, 2, 15, 16, 17, 254, 255], int(rng.integers(1, 4))))
        out.append(case(f"random_{k}", w, h, s.codes, bits, sizes=sizes, interlace=bool(rng.random() < 0.4), ext=comment(int(rng.integers(1, 40))) if rng.random() < 0.5 else b""))
    return out


@functools.lru_cache(None)
def random_streams():
    return tuple(_random(RANDOM_STREAMS, 72))


# ---- the same pixel rows as LZW TIFF strips ------------------------------------------------------------------------------------------
def tiff_strips():
    """(name, width, height, codes): the runs of every distance and the last strings cut to one pixel, as code lists that are
    TIFF's as they stand -- with 8-bit pixels GIF's clear code, end code and first entry are 256, 257, 258 too; only the
    widths and the bit order differ, and tests/_lzw_write.pack sees to those."""
    out = []
    s = W.Script(8, 64)
    s.lit(1, 2, 3)
    s.back(2)
    s.kwkwk()
    s.fill()
    out.append(("tiff_run_d2", 8, 8, s.end().codes))
    for d in range(3, 18):
        for lengths in run_lengths(d):
            for across in (False, True):
                w, h = (24, 24) if across else (16, 16)
                s = W.Script(8, w * h)
                run(s, d, lengths, pad_records=(63 - records_before_run(d, lengths)) % 64 if across else 0)
                s.fill()
                out.append((f"tiff_run_d{d}_{'_'.join(map(str, lengths))}{'_across_a_round' if across else ''}", w, h, s.end().codes))
    for n in (2, 4, 17):
        for (w, h) in ((8, 8), (17, 3)):
            s = W.Script(8, w * h)
            have = strings_up_to(s, n)
            s.fill(keep=1)
            s.code(have[n])
            out.append((f"tiff_last_string_cut_to_1_from_{n}_{w}x{h}", w, h, s.end().codes))
    return out
