"""A small deflate / zlib writer for the tests of the PNG inflate (kobato-eyes_amd/csrc/ke_png_core.h, ke_png.hip,
ke_lz_copies.h): it emits exactly the blocks, code lengths, header encoding and tokens it is GIVEN, because a compressor's
own choices cannot be steered -- zlib only ever writes a narrow, well-formed subset of RFC 1951.  Stored blocks of any length
behind a block that ends at any bit, fixed blocks, dynamic blocks with caller-given code lengths, HLIT / HDIST / HCLEN and a
caller-chosen run-length encoding of the lengths, explicit literals and (length, distance) pairs, and the zlib wrapper with
caller-given header bytes and trailer.  It does not try to compress, and it writes invalid streams as readily as valid ones.
The installed zlib is its check (tests/_png_cases.py), and every stream carries a census of what was written -- counted by
the writer, not by the decoder under test.  Written from RFC 1950 and RFC 1951."""
from __future__ import annotations

import zlib
from collections import Counter

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in range(2)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


class Bits:
    def __init__(self) -> None:
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value: int, nbits: int) -> None:
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        if self.n >= 64:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def bitpos(self) -> int:
        return len(self.out) * 8 + self.n

    def align(self) -> None:
        self.put(0, -self.bitpos() % 8)

    def raw(self, data: bytes) -> None:                           # at a byte boundary
        k = self.n >> 3
        self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little") + data
        self.acc, self.n = 0, 0

    def done(self) -> bytes:
        self.align()
        self.raw(b"")
        return bytes(self.out)


# ---- prefix codes -------------------------------------------------------------------------------------------------------
def flat_lengths(used, n: int) -> list:
    """n lengths: a complete code over the used symbols with lengths k and k + 1 (one symbol: a single 1-bit code)."""
    used = sorted(used)
    out = [0] * n
    if len(used) == 1:
        out[used[0]] = 1
        return out
    k = len(used).bit_length() - 1
    short = (1 << (k + 1)) - len(used)
    for i, s in enumerate(used):
        out[s] = k if i < short else k + 1
    return out


def kraft(lengths) -> int:
    """Sum of 2**(15 - l) over the nonzero lengths: 32768 for a complete code, less incomplete, more over-subscribed."""
    return sum(1 << (15 - l) for l in lengths if l)


def random_lengths(rng, used, n: int, limit: int) -> list:
    """A random complete code over the used symbols (two at least) from a random tree, no code longer than `limit`: leaves
    are split at random; only leaves above the limit may be split."""
    used = list(used)
    assert 2 <= len(used) <= (1 << limit)
    leaves = [1, 1]
    while len(leaves) < len(used):
        open_ = [i for i, d in enumerate(leaves) if d < limit]
        i = open_[int(rng.integers(0, len(open_)))] if rng.integers(0, 4) else max(open_, key=lambda j: leaves[j])
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    out = [0] * n
    for s, l in zip(used, leaves):
        out[s] = int(l)
    return out


def canonical(lengths) -> list:
    """symbol -> (code reversed for the LSB-first stream, length) by RFC 1951 3.2.2, None without a code.  Incomplete and
    over-subscribed sets are numbered by the same rule (an over-subscribed code word keeps its low `length` bits)."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l == 0:
            out.append(None)
            continue
        c = nxt[l] & ((1 << l) - 1)
        nxt[l] += 1
        out.append((int(format(c, f"0{l}b")[::-1], 2), l))
    return out


# ---- tokens ---------------------------------------------------------------------------------------------------------------
# int: a literal; (length, distance): a match; (length, distance, "284+31"): length 258 sent as symbol 284 with all extra
# bits set; ("sym", s): literal/length symbol s on its own; ("raw", lsym, lextra, dsym, dextra): a match by its fields
def length_fields(length: int, alt: bool = False):
    if length == 258 and alt:
        return 284, 31
    k = max(i for i, b in enumerate(LEN_BASE) if b <= length)
    assert 3 <= length <= 258 and length - LEN_BASE[k] < (1 << LEN_EXTRA[k])
    return 257 + k, length - LEN_BASE[k]


def distance_fields(dist: int):
    k = max(i for i, b in enumerate(DIST_BASE) if b <= dist)
    assert 1 <= dist <= 32768 and dist - DIST_BASE[k] < (1 << DIST_EXTRA[k])
    return k, dist - DIST_BASE[k]


_LEN_FIELDS = {n: length_fields(n) for n in range(3, 259)}
_DIST_CODE = [0] * 32769
for _k, _b in enumerate(DIST_BASE):
    for _d in range(_b, min(_b + (1 << DIST_EXTRA[_k]), 32769)):
        _DIST_CODE[_d] = _k


def token_fields(tok):
    """-> (literal/length symbol, extra value, distance symbol or None, extra value)"""
    if isinstance(tok, int):
        return tok, 0, None, 0
    if tok[0] == "sym":
        return tok[1], 0, None, 0
    if tok[0] == "raw":
        return tok[1], tok[2], tok[3], tok[4]
    ls, lx = (284, 31) if len(tok) > 2 else _LEN_FIELDS[tok[0]]
    ds = _DIST_CODE[tok[1]]
    return ls, lx, ds, tok[1] - DIST_BASE[ds]


def expand(tokens, out: bytearray) -> None:
    """What the tokens mean (RFC 1951 3.2.3), appended to `out`: the writer's own account of the intended bytes."""
    for tok in tokens:
        if isinstance(tok, int):
            out.append(tok)
        elif isinstance(tok[0], int):
            length, dist = tok[0], tok[1]
            assert dist <= len(out), "distance beyond the output so far"
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                pat = bytes(out[len(out) - dist:])
                out += (pat * (length // dist + 1))[:length]
        else:
            raise ValueError("raw symbols have no meaning of their own")


def lengths_used(tokens, n_ll: int = 286, n_d: int = 30):
    """The literal/length and distance symbols the tokens need (the end-of-block code included)."""
    ll, dd = {256}, set()
    for tok in tokens:
        ls, _, ds, _ = token_fields(tok)
        ll.add(ls)
        if ds is not None:
            dd.add(ds)
    return ll, dd


# ---- blocks ---------------------------------------------------------------------------------------------------------------
def stored(data: bytes, final: bool = False, len_=None, nlen=None) -> dict:
    return {"type": 0, "data": bytes(data), "final": final, "len": len_, "nlen": nlen}


def fixed(tokens, final: bool = False, eob: bool = True) -> dict:
    return {"type": 1, "tokens": list(tokens), "final": final, "eob": eob}


def dynamic(tokens, ll, dd, final: bool = False, eob: bool = True, hlit=None, hdist=None, hclen=None, cl=None, ops=None,
            btype: int = 2) -> dict:
    """ll / dd: code lengths by symbol (the tokens are coded with them as given).  hlit / hdist: number of lengths announced
    (default: trailing zeros trimmed, 257 and 1 at least).  ops: the run-length encoding sent, a list of (symbol, value):
    (0..15, None) one length, (16, 3..6), (17, 3..10), (18, 11..138) -- default: every length on its own.  cl: the 19 lengths of
    the code length code (default: a complete flat code over the symbols in ops).  hclen: how many of them are sent."""
    ll, dd = list(ll), list(dd)
    if hlit is None:
        hlit = max(257, max((i + 1 for i, l in enumerate(ll) if l), default=0))
    if hdist is None:
        hdist = max(1, max((i + 1 for i, l in enumerate(dd) if l), default=0))
    if ops is None:
        sent = (ll + [0] * 288)[:hlit] + (dd + [0] * 32)[:hdist]
        ops = [(l, None) for l in sent]
    if cl is None:
        used = {s for s, _ in ops}
        if len(used) == 1:                                           # a code length code of one code is incomplete: add a second
            used.add(next(s for s in (0, 1, 2) if s not in used))
        cl = flat_lengths(used, 19)
    if hclen is None:
        hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl[s]))
    return {"type": btype, "tokens": list(tokens), "ll": ll, "dd": dd, "final": final, "eob": eob, "hlit": hlit, "hdist": hdist,
            "hclen": hclen, "cl": list(cl), "ops": list(ops)}


def rle_ops(lengths, rng=None, use=(16, 17, 18)) -> list:
    """A run-length encoding of the lengths with the repeat codes in `use`; with rng the split of every run is random."""
    ops, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3 and (17 in use or 18 in use) and (rng is None or rng.integers(0, 4)):
            if 18 in use and run >= 11 and (rng is None or 17 not in use or rng.integers(0, 3)):
                r = min(run, 138) if rng is None else int(rng.integers(11, min(run, 138) + 1))
                ops.append((18, r))
            elif 17 in use:
                r = min(run, 10) if rng is None else int(rng.integers(3, min(run, 10) + 1))
                ops.append((17, r))
            else:
                r = 1
                ops.append((0, None))
            i += r
        elif i > 0 and lengths[i - 1] == v and run >= 3 and 16 in use and (rng is None or rng.integers(0, 4)):
            r = min(run, 6) if rng is None else int(rng.integers(3, min(run, 6) + 1))
            ops.append((16, r))
            i += r
        else:
            ops.append((v, None))
            i += 1
    return ops


def ops_lengths(ops) -> list:
    out = []
    for s, r in ops:
        if s < 16:
            out.append(s)
        else:
            out += [out[-1] if s == 16 else 0] * r
    return out


class Stream:
    """bits: the deflate data; census: what it holds; raw: what its tokens mean (None if some have no meaning)."""

    def __init__(self, blocks) -> None:
        self.blocks = blocks
        self.census: Counter = Counter()
        b, c = Bits(), self.census
        huffman_end = None                                            # bit offset (mod 8) where the Huffman block in front ended
        for blk in blocks:
            b.put(1 if blk["final"] else 0, 1)
            b.put(blk["type"], 2)
            if blk["type"] == 0:
                if huffman_end is not None:
                    c[f"stored_behind_bit_{huffman_end}"] += 1
                b.align()
                n = len(blk["data"])
                ln = n if blk["len"] is None else blk["len"]
                b.put(ln, 16)
                b.put((ln ^ 0xFFFF) if blk["nlen"] is None else blk["nlen"], 16)
                b.raw(blk["data"])
                c["block_stored"] += 1
                c[f"stored_{'empty' if n == 0 else 'full' if n == 65535 else 'some'}"] += 1
                if 2000 <= n < 65535:
                    c["stored_2000_or_more"] += 1
                c["stored_final" if blk["final"] else "stored_not_final"] += 1
                huffman_end = None
                continue
            if blk["type"] == 1:
                ll, dd = FIXED_LL, FIXED_D
                c["block_fixed"] += 1
            else:
                ll, dd = blk["ll"], blk["dd"]
                self._header(b, blk)
            lcode, dcode = canonical(ll), canonical(dd)
            for tok in blk["tokens"]:
                ls, lx, ds, dx = token_fields(tok)
                b.put(*lcode[ls])
                if ds is None:
                    continue
                k = ls - 257
                b.put(lx, LEN_EXTRA[k] if k < 29 else 0)
                b.put(*dcode[ds])
                b.put(dx, DIST_EXTRA[ds] if ds < 30 else 0)
                if isinstance(tok[0], int):
                    c[f"length_{tok[0]}"] += 1
                    c[f"distance_code_{ds}_{'low' if dx == 0 else 'high' if dx == (1 << DIST_EXTRA[ds]) - 1 else 'mid'}"] += 1
                    if DIST_EXTRA[ds] == 0:
                        c[f"distance_code_{ds}_high"] += 1
                    if tok[0] == 258:
                        c["length_258_as_284_31" if len(tok) > 2 else "length_258_as_285"] += 1
            if blk["eob"]:
                b.put(*lcode[256])
            huffman_end = b.bitpos() % 8
        self.bits = b.done()
        ones = [blk["type"] for blk in blocks if len(blk["data"] if blk["type"] == 0 else blk["tokens"]) == 1]
        if len(ones) == len(blocks) >= 30 and all(ones[k:k + 3] in ([0, 1, 2], [1, 2, 0], [2, 0, 1]) for k in range(len(ones) - 2)):
            c["blocks_of_one_symbol_of_alternating_types"] += 1
        try:
            out = bytearray()
            for blk in blocks:
                if blk["type"] == 0:
                    out += blk["data"]
                else:
                    expand(blk["tokens"], out)
            self.raw = bytes(out)
        except (ValueError, AssertionError):
            self.raw = None

    def _header(self, b: Bits, blk: dict) -> None:
        c = self.census
        c["block_dynamic"] += 1
        b.put(blk["hlit"] - 257, 5)
        b.put(blk["hdist"] - 1, 5)
        b.put(blk["hclen"] - 4, 4)
        for s in CL_ORDER[:blk["hclen"]]:
            b.put(blk["cl"][s], 3)
        ccode = canonical(blk["cl"])
        at = 0
        for s, r in blk["ops"]:
            b.put(*ccode[s])
            if s == 16:
                b.put(r - 3, 2)
            elif s == 17:
                b.put(r - 3, 3)
            elif s == 18:
                b.put(r - 11, 7)
            if s >= 16:
                c[f"repeat_{s}_times_{r}"] += 1
                if at < blk["hlit"] < at + r:
                    c[f"repeat_{s}_crosses_into_distances"] += 1
            at += 1 if s < 16 else r
        c[f"hclen_{blk['hclen']}"] += 1
        nl, nd = sum(1 for l in blk["ll"] if l), sum(1 for l in blk["dd"] if l)
        c[f"literal_length_symbols_{nl}"] += 1
        c[f"distance_symbols_{nd}"] += 1
        if nd == 1 and max(blk["dd"]) == 1:
            c["single_1_bit_distance_code"] += 1
        if nl == 1 and max(blk["ll"]) == 1:
            c["single_1_bit_literal_length_code"] += 1
        c[f"literal_length_longest_{max(blk['ll'])}"] += 1
        c[f"distance_longest_{max(blk['dd'], default=0)}"] += 1
        if all(s < 16 for s, _ in blk["ops"]):
            c["lengths_sent_one_by_one"] += 1
        if (blk["ll"] + [0] * 288)[blk["hlit"] - 1] == 0 or (blk["dd"] + [0] * 32)[blk["hdist"] - 1] == 0:
            c["trailing_zero_lengths_sent"] += 1
        else:
            c["trailing_zero_lengths_trimmed"] += 1


def auto_dynamic(tokens, final: bool = False, rng=None, limit: int = 15, **kw) -> dict:
    """A dynamic block around the tokens: complete codes over the symbols they use -- flat, or random trees with rng --, a
    single 1-bit distance code for one distance symbol, no distance code for none."""
    lu, du = lengths_used(tokens)
    if len(lu) == 1:
        lu.add(0 if 0 not in lu else 1)
    limit = min(15, max(limit, len(lu).bit_length() + 1))
    ll = random_lengths(rng, lu, 286, limit) if rng is not None else flat_lengths(lu, 286)
    if len(du) >= 2:
        dd = random_lengths(rng, du, 30, limit) if rng is not None else flat_lengths(du, 30)
    else:
        dd = flat_lengths(du, 30) if du else [0] * 30
    if rng is not None and "ops" not in kw:
        hlit = max(257, max(i + 1 for i, l in enumerate(ll) if l))
        hdist = max(1, max((i + 1 for i, l in enumerate(dd) if l), default=0))
        if rng.integers(0, 3) == 0:
            hlit, hdist = int(rng.integers(hlit, 287)), int(rng.integers(hdist, 31))
        kw.update(hlit=hlit, hdist=hdist, ops=rle_ops(ll[:hlit] + dd[:hdist], rng))
    return dynamic(tokens, ll, dd, final=final, **kw)


# ---- the zlib wrapper (RFC 1950) ------------------------------------------------------------------------------------------
def zlib_wrap(deflate: bytes, raw, cinfo: int = 7, flevel: int = 2, cm: int = 8, fdict: int = 0, fcheck=None, adler=None,
              tail: bytes = b"", cut: int = 0) -> bytes:
    """CMF / FLG as given (fcheck None: the value that makes the header a multiple of 31), the deflate data, the Adler-32 of
    `raw` (or `adler` as given), bytes behind the trailer; `cut` bytes taken off the end."""
    cmf = (cinfo << 4) | cm
    flg = (flevel << 6) | (fdict << 5)
    flg |= (31 - ((cmf << 8) | flg) % 31) % 31 if fcheck is None else fcheck
    if adler is None:
        adler = zlib.adler32(raw if raw is not None else b"")
    z = bytes([cmf, flg]) + deflate + adler.to_bytes(4, "big") + tail
    return z[:len(z) - cut] if cut else z


# ---- what the copies of a token list look like to a decoder that records them and makes them later -----------------------
def copy_census(tokens, first: int = 0) -> Counter:
    """Features of the matches in the order they are made, from the tokens alone; `first`: output bytes in front of them."""
    c: Counter = Counter()
    pos, recs, prev_lit = first, [], True
    ends_lit = {}                                                     # index of a copy -> a literal follows it
    for tok in tokens:
        if isinstance(tok, int):
            if recs and len(recs) - 1 not in ends_lit:
                ends_lit[len(recs) - 1] = True
            pos += 1
            prev_lit = True
            continue
        length, dist = tok[0], tok[1]
        recs.append((pos, dist, length, prev_lit))
        pos += length
        prev_lit = False
    total = pos
    c[f"copies_over_{64 * (min(len(recs) - 1, 191) // 64)}"] += 1 if recs else 0
    run, broken = 0, False
    for k, (dst, dist, length, lit_before) in enumerate(recs):
        if dist < length:
            c[f"overlap_distance_{dist}"] += 1
        c[f"distance_{dist}_length_{length}"] += 1
        if dst + length == total:
            c["copy_ends_with_the_output"] += 1
        if lit_before and ends_lit.get(k):
            c[f"copy_from_mod4_{dst % 4}_to_mod4_{(dst + length) % 4}_between_literals"] += 1
        cont = k > 0 and recs[k - 1][1] == dist and recs[k - 1][0] + recs[k - 1][2] == dst
        if cont:
            run += 1
        else:
            if k > 0 and recs[k - 1][1] == dist and dist <= 16 and recs[k - 1][0] + recs[k - 1][2] + 1 == dst:
                c["run_broken_by_one_literal"] += 1
            run = 1
            if dist <= 16 and dst == dist:
                c["run_head_reads_from_offset_0"] += 1
        nxt = recs[k + 1] if k + 1 < len(recs) else None
        if run >= 2 and not (nxt and nxt[1] == dist and nxt[0] == dst + length):
            c[f"run_of_{run}_copies_of_distance_{dist}"] += 1
        # blockers: an earlier copy of the same group of 64 whose output this copy reads
        for back in range(1, (k % 64) + 1):
            p = recs[k - back]
            if p[0] < dst - dist + min(dist, length) and p[0] + p[2] > dst - dist:
                c[f"source_written_{back}_copies_earlier"] += 1
    # a chain: every copy reads what the copy in front of it wrote, too far back to continue its run
    chain = best = 0
    for k in range(1, len(recs)):
        p, (dst, dist, length, _) = recs[k - 1], recs[k]
        chain = chain + 1 if dist > 16 and p[0] < dst - dist + min(dist, length) and p[0] + p[2] > dst - dist and p[0] + p[2] == dst else 0
        best = max(best, chain)
    if best >= 100:
        c["chain_of_100_dependent_copies"] += 1
    if recs and all(r[2] == 3 for r in recs) and recs[0][0] <= first + 8 and recs[-1][0] + 3 == total:
        c["only_length_3_copies_behind_a_short_head"] += 1
    return c
