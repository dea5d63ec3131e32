"""A coefficient-level JPEG writer for the decoder tests: quantised coefficients, quantisation tables and Huffman tables of ANY
shape in, a baseline (SOF0 / SOF1) or progressive (SOF2) file out -- it emits exactly what it is told, as tests/_lzw_write.py
and tests/_deflate_write.py do for their formats, and returns the facts of what it wrote (code lengths used per table, the
file position of every stuffed FF 00, restart marker and of the EOI, the end-of-band runs) for the case families to assert
their coverage on.  The entropy coding follows T.81 F.1.2 (sequential) and Annex G as libjpeg's jchuff.c / jcphuff.c do,
end-of-band runs and their flush at restarts and at the end of a scan included.

A file is written in two steps: the scans become token lists (Huffman symbols by table, raw bits, restarts), then the tables
are resolved -- `htables` is a dict {(class, id): Table} or a callable (scan index, class, id, Counter of the symbols the scan
draws from that table) -> Table, so a table can be shaped on the symbols a coefficient set really uses -- and the tokens are
packed into bytes."""
from __future__ import annotations

import struct
from collections import Counter
from types import SimpleNamespace


# ---- Huffman tables ----------------------------------------------------------------------------------------------------------------
class Table:
    """A DHT payload -- 16 counts, the symbols in code order -- and the canonical codes of T.81 Annex C: {symbol: (code, length)}.
    Nothing is checked here (the refused-table cases need bad ones); `valid()` is jdhuff.c's rule."""

    def __init__(self, counts, syms, marks=None):
        self.counts, self.syms, self.marks = [int(c) for c in counts], [int(s) for s in syms], dict(marks or {})
        self.codes = {}
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(self.counts[length - 1]):
                if k < len(self.syms):
                    self.codes.setdefault(self.syms[k], (code, length))
                code += 1
                k += 1
            code <<= 1

    @property
    def payload(self) -> bytes:
        return bytes(self.counts) + bytes(self.syms)

    def valid(self, dc: bool = False) -> bool:
        """jpeg_make_d_derived_tbl: a prefix code whose codes of every length leave the all-ones code free (and symbols 0..15 in
        a DC table); get_dht: as many symbols as the counts say, 256 at most."""
        code = 0
        for length in range(1, 17):
            code += self.counts[length - 1]
            if self.counts[length - 1] and code >= 1 << length:
                return False
            if code > 1 << length:
                return False
            code <<= 1
        if sum(self.counts) != len(self.syms) or len(self.syms) > 256 or len(set(self.syms)) != len(self.syms):
            return False
        return not dc or all(s <= 15 for s in self.syms)

    def lengths(self):
        return {s: n for s, (_, n) in self.codes.items()}


def table(symbols, lengths, marks=None, dc: bool = False) -> Table:
    """The table that gives symbols[i] a code of lengths[i] bits (canonical: shorter first, the given order within a length)."""
    order = sorted(range(len(symbols)), key=lambda i: lengths[i])
    counts = [0] * 16
    for n in lengths:
        assert 1 <= n <= 16
        counts[n - 1] += 1
    t = Table(counts, [symbols[i] for i in order], marks)
    assert t.valid(dc), (counts, symbols)
    return t


def _kraft(lengths) -> int:
    return sum(1 << (16 - n) for n in lengths)            # < 65536 <=> a prefix code that leaves the all-ones code free


# the shapes: each takes the symbols the table must hold, most wanted first
def ladder(symbols, lo: int, dc: bool = False) -> Table:
    """One code per length from `lo` upward; what does not fit below gets 16 bits."""
    lengths = [min(lo + i, 16) for i in range(len(symbols))]
    return table(symbols, lengths, dc=dc)


def all_sixteen(symbols, dc: bool = False) -> Table:
    return table(symbols, [16] * len(symbols), dc=dc)


def edge_9_10(symbols, dc: bool = False) -> Table:
    """Codes of 9 and of 10 bits on either side of the 9-bit look-up's boundary: symbols[0] gets the LARGEST 9-bit code of the
    table, symbols[1] the smallest 10-bit one (the code right behind it); the others alternate between the lengths, and seven
    short codes of 1..7 bits in front (given to the last symbols) push the 9-bit codes up to 0x1FC.. so that the 10-bit ones
    begin with nine ones but for the last bit."""
    n = len(symbols)
    assert n >= 2
    rest = list(symbols[2:])
    short = [rest.pop() for _ in range(min(7, max(0, len(rest) - 2)))]
    nine = [s for i, s in enumerate(rest) if i % 2 == 0] + [symbols[0]]
    ten = [symbols[1]] + [s for i, s in enumerate(rest) if i % 2 == 1]
    syms = short + nine + ten
    lengths = [1 + i for i in range(len(short))] + [9] * len(nine) + [10] * len(ten)
    while _kraft(lengths) >= 65536:                       # too many for the room behind the short codes: drop short codes
        k = lengths.index(min(lengths))
        lengths[k] = 10
        syms.append(syms.pop(k))
        lengths.append(lengths.pop(k))
    return table(syms, lengths, marks={"last9": symbols[0], "first10": symbols[1]}, dc=dc)


def single(symbol: int, length: int) -> Table:
    return table([symbol], [length])


def _spread(symbols, n: int):
    """All symbols 0 .. n - 1, the wanted ones (most wanted first) at evenly spaced places of the code order: their codes are of
    every length the shape has, and their indices reach the end of the table."""
    wanted = list(symbols)
    places = {round(i * (n - 1) / max(len(wanted) - 1, 1)): s for i, s in enumerate(wanted)}
    assert len(places) == len(wanted)
    rest = iter(s for s in range(n) if s not in set(wanted))
    return [places[i] if i in places else next(rest) for i in range(n)]


def full_256(symbols) -> Table:
    """All 256 symbols in an AC table, 128 at 8 bits, then 9, ... the last two at 16; the wanted ones spread over all of it."""
    lengths = [8] * 128 + [9] * 64 + [10] * 32 + [11] * 16 + [12] * 8 + [13] * 4 + [14] * 2 + [16] * 2
    return table(_spread(symbols, 256), lengths)


def dc_full(symbols, n: int) -> Table:
    """A DC table with n (12 or 16) symbols at lengths 2, 3, 4, ... and 16 for the rest; the wanted ones spread over all of it."""
    return table(_spread(symbols, n), [min(2 + i, 16) for i in range(n)], dc=True)


def inverted(counter: Counter, dc: bool = False) -> Table:
    """The symbols a coefficient set uses most get the longest codes: 16, 16, 15, 15, ... down to 9."""
    syms = [s for s, _ in sorted(counter.items(), key=lambda kv: (-kv[1], kv[0]))]
    return table(syms, [max(16 - i // 2, 9) for i in range(len(syms))], dc=dc)


def random(rng, symbols, lo: int, dc: bool = False) -> Table:
    """Random Kraft-valid lengths of at least `lo`."""
    symbols = list(symbols)
    lengths = [int(v) for v in rng.integers(lo, 17, len(symbols))]
    while _kraft(lengths) >= 65536:
        k = int(rng.integers(0, len(lengths)))
        if lengths[k] < 16:
            lengths[k] += 1
    order = rng.permutation(len(symbols))
    return table([symbols[i] for i in order], [lengths[i] for i in order], dc=dc)


# ---- bits --------------------------------------------------------------------------------------------------------------------------
class _Bits:
    """Packs bits behind `out` (the file so far: positions are file positions) with byte stuffing."""

    def __init__(self, out: bytearray, facts):
        self.out, self.facts, self.acc, self.n = out, facts, 0, 0

    def put(self, value: int, length: int):
        if length == 0:
            return
        self.acc = (self.acc << length) | (value & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.out.append(byte)
            if byte == 0xFF:
                self.facts.stuffed.append(len(self.out) - 1)
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self, ones: bool):
        self.facts.pad_bits.append((8 - self.n) % 8)
        if self.n:
            self.put((1 << (8 - self.n)) - 1 if ones else 0, 8 - self.n)


def category(v: int) -> int:
    return int(abs(v)).bit_length()


def _magnitude(v: int, size: int) -> int:
    return v if v >= 0 else v + (1 << size) - 1


# ---- scans into tokens: ("s", class, table id, symbol) / ("b", value, bits) / ("r",) -----------------------------------------------
def _geometry(width, height, comps):
    if len(comps) == 1:                                   # a single component is never interleaved: its factors are ignored
        return 1, 1, -(-width // 8), -(-height // 8)
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    return hmax, vmax, -(-width // (8 * hmax)), -(-height // (8 * vmax))


def _seq_block(tok, blk, td, ta, pred, zrl_tail):
    diff = int(blk[0]) - pred
    size = category(diff)
    tok += [("s", 0, td, size), ("b", _magnitude(diff, size), size)]
    nz = [k for k in range(1, 64) if blk[k]]
    last = nz[-1] if nz else 0
    run = 0
    for k in range(1, last + 1):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            tok.append(("s", 1, ta, 0xF0))
            run -= 16
        size = category(v)
        tok += [("s", 1, ta, (run << 4) | size), ("b", _magnitude(v, size), size)]
        run = 0
    if last < 63:                                         # (coefficient 63 set: the block is complete, no end-of-block)
        for _ in range(min(zrl_tail, (62 - last) // 16)):  # ZRLs where an EOB would do: the position stays below 64
            tok.append(("s", 1, ta, 0xF0))
        tok.append(("s", 1, ta, 0x00))
    return int(blk[0])


def _seq_tokens(width, height, comps, coefs, restart, zrl_tail, override, stop_after):
    hmax, vmax, mcus_x, mcus_y = _geometry(width, height, comps)
    tok, pred, at = [], [0] * len(comps), 0
    for my in range(mcus_y):
        for mx in range(mcus_x):
            if stop_after is not None and at >= stop_after:
                return tok
            if restart and at and at % restart == 0:
                tok.append(("r",))
                pred = [0] * len(comps)
            for c, comp in enumerate(comps):
                hs, vs = (comp[1], comp[2]) if len(comps) > 1 else (1, 1)
                for by in range(vs):
                    for bx in range(hs):
                        row, col = my * vs + by, mx * hs + bx
                        if (c, row, col) in override:     # the block as a list of tokens, whatever they say
                            tok += [t if t[0] == "b" else ("s", t[1], comp[4 + t[1]], t[2]) for t in override[(c, row, col)]]
                            continue
                        z = zrl_tail(c, row, col) if callable(zrl_tail) else zrl_tail
                        pred[c] = _seq_block(tok, coefs[c][row, col], comp[4], comp[5], pred[c], z)
            at += 1
    return tok


class _EobRun:
    """jcphuff.c's EOBRUN / BE state: the run and the correction bits that wait behind its symbol."""

    def __init__(self, tok, ta, limit, facts):
        self.tok, self.ta, self.limit, self.facts, self.run, self.bits = tok, ta, limit, facts, 0, []

    def emit(self) -> int:
        """-> 1 if a run was written."""
        had = int(self.run > 0)
        if self.run:
            n = self.run.bit_length() - 1
            self.tok.append(("s", 1, self.ta, n << 4))
            self.tok.append(("b", self.run & ((1 << n) - 1), n))
            self.facts.eobruns.append(self.run)
            self.facts.eobrun_pending.append(len(self.bits))
            self.run = 0
        self.tok += [("b", b, 1) for b in self.bits]
        self.bits = []
        return had

    def block_ends(self, pending):
        self.run += 1
        self.bits += pending
        if self.run >= self.limit or len(self.bits) > 937:   # MAX_CORR_BITS - DCTSIZE2 + 1
            self.emit()


def _prog_tokens(width, height, comps, coefs, scan, restart, max_eobrun, facts):
    members, ss, se, ah, al = scan[:5]
    hmax, vmax, mcus_x, mcus_y = _geometry(width, height, comps)
    tok, at = [], 0
    if ss == 0:
        pred = [0] * len(comps)
        if len(members) > 1:
            units = [(my, mx) for my in range(mcus_y) for mx in range(mcus_x)]
        else:
            c = members[0]
            hs1, vs1 = (comps[c][1], comps[c][2]) if len(comps) > 1 else (1, 1)
            cw, ch = -(-width * hs1 // hmax), -(-height * vs1 // vmax)
            units = [(by, bx) for by in range(-(-ch // 8)) for bx in range(-(-cw // 8))]
        for (uy, ux) in units:
            if restart and at and at % restart == 0:
                tok.append(("r",))
                pred = [0] * len(comps)
            for c in members:
                hs, vs = (comps[c][1], comps[c][2]) if len(members) > 1 else (1, 1)
                for by in range(vs):
                    for bx in range(hs):
                        v = int(coefs[c][uy * vs + by, ux * hs + bx, 0])
                        if ah == 0:
                            t = v >> al                      # arithmetic shift, as jcphuff does for DC
                            diff = t - pred[c]
                            pred[c] = t
                            size = category(diff)
                            tok += [("s", 0, comps[c][4], size), ("b", _magnitude(diff, size), size)]
                        else:
                            tok.append(("b", (v >> al) & 1, 1))
            at += 1
        return tok
    c = members[0]
    ta = comps[c][5]
    hs1, vs1 = (comps[c][1], comps[c][2]) if len(comps) > 1 else (1, 1)
    cw, ch = -(-width * hs1 // hmax), -(-height * vs1 // vmax)
    eob = _EobRun(tok, ta, max_eobrun, facts)
    for by in range(-(-ch // 8)):
        for bx in range(-(-cw // 8)):
            if restart and at and at % restart == 0:
                facts.eobrun_flushed_at_restart += eob.emit()   # a run is flushed at a restart
                tok.append(("r",))
            at += 1
            blk = coefs[c][by, bx]
            if ah == 0:
                run = 0
                for k in range(ss, se + 1):
                    v = int(blk[k])
                    t = (abs(v) >> al) * (1 if v >= 0 else -1)
                    if t == 0:
                        run += 1
                        continue
                    eob.emit()
                    while run > 15:
                        tok.append(("s", 1, ta, 0xF0))
                        run -= 16
                    size = category(t)
                    tok += [("s", 1, ta, (run << 4) | size), ("b", _magnitude(t, size), size)]
                    run = 0
                if run > 0:
                    eob.block_ends([])
            else:
                absval = [abs(int(blk[k])) >> al for k in range(64)]
                last_new = max([k for k in range(ss, se + 1) if absval[k] == 1], default=-1)
                run, pending = 0, []
                for k in range(ss, se + 1):
                    t = absval[k]
                    if t == 0:
                        run += 1
                        continue
                    while run > 15 and k <= last_new:
                        eob.emit()
                        tok.append(("s", 1, ta, 0xF0))
                        tok += [("b", b, 1) for b in pending]
                        pending = []
                        run -= 16
                    if t > 1:                                # already nonzero: one more bit of it, sent behind the next symbol
                        pending.append(t & 1)
                        continue
                    eob.emit()
                    tok += [("s", 1, ta, (run << 4) | 1), ("b", 1 if int(blk[k]) >= 0 else 0, 1)]
                    tok += [("b", b, 1) for b in pending]
                    pending = []
                    run = 0
                if run > 0 or pending:
                    eob.block_ends(pending)
    facts.eobrun_at_scan_end += eob.emit()                   # ... and at the end of the scan
    return tok


# ---- the file ----------------------------------------------------------------------------------------------------------------------
def segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack(">H", 2 + len(payload)) + payload


JFIF = segment(0xE0, struct.pack(">5sBBBHHBB", b"JFIF\0", 1, 1, 0, 1, 1, 0, 0))


def adobe(transform: int) -> bytes:
    return segment(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, transform))


def com(n: int) -> bytes:
    """A COM segment of n bytes in all (n = 0: none; n >= 4)."""
    assert n == 0 or n >= 4
    return segment(0xFE, b"c" * (n - 4)) if n else b""


def write(width, height, comps, coefs, qtables, htables, *, sof=0xC0, script=None, restart=0, pad_ones=True, jfif=True,
          adobe_transform=None, leading=b"", dht_layout="each", dht_behind_sof=True, dht_twice=False, extra_tables=False,
          dqt_behind_sof=False, dri=None, zrl_tail=0, override=None, stop_after=None, max_eobrun=1, before_marker=None,
          rst_number=None, raw_dht=None, frame_factors=None):
    """comps: [(id, hs, vs, tq, td, ta)]; coefs[c]: int array [block rows][block columns][64], zigzag order, padded to whole MCUs;
    qtables: {id: 64 steps in zigzag order} (or a list); htables: see the module's docstring.
    sof: 0xC0 / 0xC1 (one interleaved scan) or 0xC2 with script = [(component indices, ss, se, ah, al[, restart interval])].
    restart: the interval (progressive: of every scan that does not bring its own); dri: the DRI segments written in front of
    the SOF instead of one for `restart` (the last one must say `restart`); pad_ones: the bits that fill a last byte.
    leading: segments put right in front of the first SOS.  dht_layout: "each" / "one" segment; dht_twice: every table is
    defined twice, the first time with other contents; extra_tables: unused tables under the ids the scan leaves free.
    zrl_tail: ZRLs written in front of every EOB where they fit (an int or f(c, row, col)); override: {(c, row, col): tokens}
    for blocks written symbol by symbol -- ("s", class, symbol) / ("b", value, bits); stop_after: the data ends after that many
    MCUs; before_marker: {restart ordinal or "eoi": raw bytes in front of that marker}; rst_number: f(ordinal) -> the number a
    restart marker carries; raw_dht: DHT segments written as given instead of the tables; frame_factors: the sampling bytes
    of the frame header where they are not the components' (a gray file that states 2 x 2).
    max_eobrun: the longest end-of-band run (1 = an EOB per block, 32 767 = libjpeg's).
    -> (file, facts)."""
    facts = SimpleNamespace(stuffed=[], restarts=[], eoi=None, eobruns=[], eobrun_pending=[], eobrun_flushed_at_restart=0, eobrun_at_scan_end=0, pad_bits=[],
                            scan_offsets=[], scan_ends=[], symbols={}, lengths={}, tables={}, reads=[])
    qtables = dict(enumerate(qtables)) if not isinstance(qtables, dict) else qtables
    override, before_marker = override or {}, before_marker or {}
    progressive = sof == 0xC2
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += JFIF
    if adobe_transform is not None:
        out += adobe(adobe_transform)
    dqt = b"".join(segment(0xDB, bytes([k]) + bytes(int(v) for v in q)) for k, q in qtables.items())
    frame = struct.pack(">BHHB", 8, height, width, len(comps))
    for k, comp in enumerate(comps):
        frame += bytes([comp[0], frame_factors[k] if frame_factors else (comp[1] << 4) | comp[2], comp[3]])

    scans = script if progressive else [(list(range(len(comps))), 0, 63, 0, 0)]
    per_scan = []
    for scan in scans:
        ri = scan[5] if len(scan) > 5 else restart
        if progressive:
            tok = _prog_tokens(width, height, comps, coefs, scan, ri, max_eobrun, facts)
        else:
            tok = _seq_tokens(width, height, comps, coefs, ri, zrl_tail, override, stop_after)
        per_scan.append((scan, ri, tok))

    def resolve(si, tok):
        used = {}
        for t in tok:
            if t[0] == "s":
                used.setdefault((t[1], t[2]), Counter())[t[3]] += 1
        return {key: (htables(si, key[0], key[1], cnt) if callable(htables) else htables[key]) for key, cnt in sorted(used.items())}, used

    def dht_segments(tabs, current):
        pieces = []
        for key, t in tabs.items():
            if current.get(key) is t:
                continue
            if dht_twice:                                 # the first definition: the same symbols, all at 16 bits
                pieces.append(bytes([(key[0] << 4) | key[1]]) + all_sixteen(t.syms).payload)
            pieces.append(bytes([(key[0] << 4) | key[1]]) + t.payload)
            current[key] = t
        if extra_tables:
            for cls in (0, 1):
                for tid in (2, 3):
                    if (cls, tid) not in current:
                        pieces.append(bytes([(cls << 4) | tid]) + ladder(list(range(12)), 3).payload)
                        current[(cls, tid)] = None
        if not pieces:
            return b""
        return segment(0xC4, b"".join(pieces)) if dht_layout == "one" else b"".join(segment(0xC4, p) for p in pieces)

    current = {}
    resolved = [resolve(si, tok) for si, (_, _, tok) in enumerate(per_scan)]
    first_tabs = resolved[0][0]
    if progressive and not callable(htables):
        first_tabs = dict(htables)                        # every table of the file in front of the first scan
    dht0 = b"".join(raw_dht) if raw_dht is not None else dht_segments(first_tabs, current)
    if not dqt_behind_sof:
        out += dqt
    if not dht_behind_sof:
        out += dht0
    dri_now = 0
    for n in ([restart] if dri is None and not progressive and restart else (dri or [])):
        out += segment(0xDD, struct.pack(">H", n))
        dri_now = n
    out += segment(sof, frame)
    if dqt_behind_sof:
        out += dqt
    if dht_behind_sof:
        out += dht0
    out += leading

    for si, (scan, ri, tok) in enumerate(per_scan):
        tabs, used = resolved[si]
        if si:
            out += dht_segments(tabs, current)
        if ri != dri_now and (progressive or dri is None):
            out += segment(0xDD, struct.pack(">H", ri))
            dri_now = ri
        members, ss, se, ah, al = scan[:5]
        out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * len(members), len(members))
        for c in members:
            out += bytes([comps[c][0], (comps[c][4] << 4) | comps[c][5]])
        out += bytes([ss, se, (ah << 4) | al])
        facts.scan_offsets.append(len(out))
        bits = _Bits(out, facts)
        ordinal, in_scan = len(facts.restarts), 0
        reads = []                                        # bits per Huffman symbol with what follows it: a decoder's refill points
        facts.reads.append(reads)
        for t in tok:
            if t[0] == "s":
                code, n = tabs[(t[1], t[2])].codes[t[3]]
                bits.put(code, n)
                reads.append(n)
                facts.lengths.setdefault((si, t[1], t[2]), Counter())[n] += 1
            elif t[0] == "b":
                bits.put(t[1], t[2])
                if reads:
                    reads[-1] += t[2]
            else:
                bits.flush(pad_ones)
                out += before_marker.get(ordinal, b"")
                facts.restarts.append(len(out))
                out += bytes([0xFF, 0xD0 + ((rst_number(ordinal) if rst_number else in_scan) & 7)])
                in_scan += 1
                ordinal += 1
        bits.flush(pad_ones)
        facts.scan_ends.append(len(out))
        for key, cnt in used.items():
            facts.symbols[(si,) + key] = cnt
            facts.tables[(si,) + key] = tabs[key]
    out += before_marker.get("eoi", b"")
    facts.eoi = len(out)
    out += b"\xff\xd9"
    return bytes(out), facts

