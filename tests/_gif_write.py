"""A GIF LZW writer for the tests that emits exactly the codes it is given, LSB-first, at the width a reader of Pillow's
GifDecode.c kind expects at that point, cut into sub-blocks from a given list of sizes -- so that streams no greedy encoder
produces can be built: no opening clear code, clear codes anywhere and in a row, a code that is the entry being built
(KwKwK) at a chosen width, a parse that is not the longest match, a last string cut to one pixel.  The writer counts what it
wrote (a Counter); `Script` builds a code list step by step while it follows what a reader knows, `encode` turns given pixels
into codes with the choices a greedy encoder never makes."""
from __future__ import annotations

from collections import Counter

LENGTHS = (2, 3, 15, 16, 17, 511, 512, 513, 514, 515, 1025, 1026, 1027)       # the piece-splitting and copy boundaries


class Reader:
    """What the reader knows after the codes so far: the next free entry, the code width, every entry as (where its string
    begins in the output, its length), and the output itself.  `want`: the frame's pixels; strings are cut there and what
    comes behind is not decoded (only its width is tracked on, as if it were)."""

    def __init__(self, bits: int, want: int | None = None):
        self.bits, self.clear, self.end, self.want = bits, 1 << bits, (1 << bits) + 1, want
        self.out = bytearray()
        self.dead = False              # a code no reader accepts went by: what follows is bits, not codes
        self.reset()

    def reset(self):
        self.next, self.width, self.fresh = self.clear + 2, self.bits + 1, True
        self.entry, self.code_at, self.last = {}, {}, None

    def full(self):
        return self.want is not None and len(self.out) >= self.want

    def expands(self, code):
        """(from, length) of a code that is a string now, None for a literal; ValueError for a code no reader accepts."""
        if code < self.clear:
            return None
        if self.fresh or code > self.next or code <= self.end or (code == self.next and self.next >= 4096):
            raise ValueError(code)
        if code == self.next:
            return self.last[0], self.last[1] + 1
        return self.entry[code]

    def feed(self, code):
        """-> (kind, width, length, distance): kind in clear / end / literal / string / kwkwk / bad / behind."""
        width = self.width
        if self.dead or self.full():
            return ("behind", width, 0, 0)
        if code == self.clear:
            self.reset()
            return ("clear", width, 0, 0)
        if code == self.end:
            return ("end", width, 0, 0)
        at = len(self.out)
        try:
            s = self.expands(code)
        except ValueError:
            self.dead = True
            return ("bad", width, 0, 0)
        kind = "literal" if s is None else "kwkwk" if code == self.next else "string"
        if s is None:
            self.out.append(code)
            n, dist = 1, 0
        else:
            n, dist = s[1], at - s[0]
            head = bytes(self.out[s[0]:s[0] + min(n, dist)])     # a string that runs into its own output repeats its head
            self.out += (head * (n // len(head) + 1))[:n]
        if self.fresh:
            self.fresh = False
        elif self.next < 4096:
            self.entry[self.next] = (self.last[0], self.last[1] + 1)
            self.code_at[self.last[0]] = self.next
            if self.next == (1 << self.width) - 1 and self.width < 12:
                self.width += 1
            self.next += 1
        self.last = (at, n)
        if self.want is not None and len(self.out) > self.want:
            del self.out[self.want:]
        return (kind, width, n, dist)


def pack(codes, bits: int) -> bytes:
    """The codes as bytes, LSB-first, the last byte padded with zeros."""
    raw, _ = _pack(codes, bits, None)
    return raw


def _pack(codes, bits, want):
    r, census = Reader(bits, want), Counter()
    acc = n = 0
    raw, starts = bytearray(), []            # starts: the bit each code begins at
    clears, since_clear, prev_grew, strings = 0, None, False, set()
    bitpos = 0
    if codes and codes[0] != r.clear:
        census["no_opening_clear"] += 1
    last_kind = None
    for code in codes:
        before_next, before_width, fresh, left = r.next, r.width, r.fresh, (None if want is None else want - len(r.out))
        kind, width, length, dist = r.feed(code)
        starts.append((bitpos, width))
        acc |= code << n
        n += width
        bitpos += width
        while n >= 8:
            raw.append(acc & 255)
            acc >>= 8
            n -= 8
        if kind == "clear":
            clears += 1
            census[f"clear_at_width_{width}"] += 1
            if clears in (2, 3):
                census[f"clears_in_a_row_{clears}"] += 1
            if prev_grew:
                census["clear_when_the_width_has_just_grown"] += 1
            if not fresh and before_next == (1 << before_width) - 1 and before_width < 12:
                census["clear_one_code_before_the_width_grows"] += 1
            since_clear = 0
        elif kind == "behind":
            census["clear_behind_the_last_pixel"] += code == r.clear and last_kind != "behind"
            census["end_code_behind_the_last_pixel"] += code == r.end
        elif kind in ("literal", "string", "kwkwk"):
            clears = 0
            since_clear = None if since_clear is None else since_clear + 1
            census[f"codes_with_a_full_table_bits_{bits}"] += before_next == 4096
            if kind == "kwkwk":
                census[f"kwkwk_at_width_{width}"] += 1
                census["kwkwk_second_code_after_a_clear"] += since_clear == 2
                census["kwkwk_at_next_4095"] += before_next == 4095
            if kind == "string":
                census["code_equal_to_the_newest_entry"] += code == before_next - 1
                census["entry_used_4000_pixels_back"] += dist >= 4000
            if kind != "literal":
                how = "kwkwk" if kind == "kwkwk" else "old_entry" if dist > 16 else None
                if how and (length in LENGTHS or length > 3000):
                    census[f"length_{length if length <= 3000 else 'above_3000'}_{how}"] += 1
                census["length_17_at_distance_16"] += length > 16 and dist <= 16
            if r.next > before_next and r.entry[before_next][1] <= 32:
                s = bytes(r.out[r.entry[before_next][0]:r.entry[before_next][0] + r.entry[before_next][1]])
                if len(s) == r.entry[before_next][1]:
                    census["duplicate_string_in_the_dictionary"] += s in strings
                    strings.add(s)
            if want is not None and left is not None and length >= left:      # the frame's last string
                census["last_string_ends_at_the_last_pixel"] += length == left and kind != "literal"
                census["last_code_is_a_literal"] += kind == "literal"
                census["last_string_cut_to_1"] += left == 1 and length > 1
                census["last_string_cut_to_2"] += left == 2 and length > 2
                census["last_string_cut_from_above_513"] += length > 513 and length > left
        elif kind == "end":
            census["end_code_before_the_last_pixel"] += 1
        if kind == "clear":
            strings = set()
        prev_grew = r.width > before_width
        last_kind = kind
    if n:
        raw.append(acc & 255)
    if want is not None and len(r.out) >= want and not census["end_code_behind_the_last_pixel"]:
        census["no_end_code"] += 1
    return bytes(raw), (census, starts, r)


def stream(codes, bits: int, *, sizes=(255,), terminator=True, want=None):
    """-> (the minimum code size byte, the sub-blocks, the terminator; the census of what was written).  The sub-blocks take
    their sizes from `sizes`, cycled; the last one is what is left."""
    raw, (census, starts, _) = _pack(codes, bits, want)
    body, cuts = bytearray([bits]), []
    o = k = 0
    while o < len(raw):
        size = min(sizes[k % len(sizes)], len(raw) - o)
        census[f"sub_block_of_{size}"] += 1
        census[f"size_byte_at_window_offset_{(len(body) - 1) % 16}"] += 1     # counted from the first size byte: the window's base
        body += bytes([size]) + raw[o:o + size]
        o += size
        k += 1
        cuts.append(8 * o)
    at = 0
    for cut in cuts[:-1]:                                         # codes that lie across a sub-block's end
        while at < len(starts) and starts[at][0] + starts[at][1] <= cut:
            at += 1
        if at < len(starts) and starts[at][0] < cut:
            census[f"code_split_after_{cut - starts[at][0]}_bits"] += 1
    if terminator:
        body.append(0)
    else:
        census["no_block_terminator"] += 1
    return bytes(body), census


class Script:
    """A code list written step by step, with the reader's state at hand."""

    def __init__(self, bits: int, want: int | None = None, *, open_clear=True):
        self.r, self.codes = Reader(bits, want), []
        if open_clear:
            self.code(self.r.clear)

    def code(self, c):
        self.codes.append(c)
        return self.r.feed(c)

    def lit(self, *values):
        for v in values:
            self.code(v % self.r.clear)

    def clear(self, times=1):
        for _ in range(times):
            self.code(self.r.clear)

    def kwkwk(self):
        assert not self.r.fresh and self.r.next < 4096
        return self.code(self.r.next)

    def back(self, d):
        """The entry whose string begins d pixels back."""
        return self.code(self.r.code_at[len(self.r.out) - d])

    def lits_until(self, next_, start=0):
        """Literals (each adds an entry) until the next free entry is next_."""
        k = start
        if self.r.fresh:
            self.lit(k)
            k += 1
        while self.r.next < next_:
            self.lit(k)
            k += 1

    def left(self):
        return self.r.want - len(self.r.out)

    def fill(self, keep=0, start=0):
        """Literals up to `keep` pixels before the frame's end."""
        k = start
        while self.left() > keep:
            self.lit(k * 7 + 1)
            k += 1

    def end(self):
        self.codes.append(self.r.end)
        return self


def encode(pixels, bits: int, *, open_clear=True, clear_at=(), max_len=None, d_back=None, rng=None, end=True):
    """Pixels -> codes.  By default the longest match; max_len: never a string longer than that; d_back: the entry that begins
    d pixels back wherever there is one that fits; rng: any of the codes valid at that point (a literal, every entry that
    matches what comes -- duplicates too -- the entry being built where it matches), drawn by rng; clear_at: a clear code
    whenever the reader's next free entry is one of these."""
    want = len(pixels)
    s = Script(bits, want, open_clear=open_clear)
    r = s.r
    px = bytes(pixels)
    while len(r.out) < want:
        p = len(r.out)
        if not r.fresh and r.next in clear_at:
            s.clear()
        cands = [(1, px[p])]
        if not r.fresh:
            for code, (pos, n) in r.entry.items():
                if r.out[pos] == px[p] and (max_len is None or n <= max_len) and n <= want - p and r.out[pos:pos + n] == px[p:p + n]:
                    cands.append((n, code))
            if r.next < 4096:
                pos, n = r.last[0], r.last[1] + 1
                if (max_len is None or n <= max_len) and n <= want - p and (r.out[pos:pos + n - 1] + r.out[pos:pos + 1]) == px[p:p + n]:
                    cands.append((n, r.next))
        pick = None
        if d_back is not None and not r.fresh and p - d_back in r.code_at:
            pick = next((c for c in cands if c[1] == r.code_at[p - d_back]), None)
        if pick is None:
            pick = cands[int(rng.integers(0, len(cands)))] if rng is not None else max(cands)
        s.code(pick[1])
    assert bytes(r.out) == px
    if end:
        s.end()
    return s.codes
