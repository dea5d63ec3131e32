"""A TIFF LZW writer for the tests that emits exactly the codes it is given, MSB-first, at the width a libtiff-style reader
expects at that point -- so that streams libtiff's own writer never produces can be built: a clear code in mid-strip, a table
run to its last entries, no end code, bytes behind it -- and invalid ones: no opening clear code, a code beyond the table,
the "late change" width rule, libtiff's old-style LSB-first packing.  Plus a PackBits writer in the same spirit."""
from __future__ import annotations

CLEAR, EOI, FIRST = 256, 257, 258


def widths(codes, *, early=True):
    """The width each code is written with, as a reader tracks it: 9 bits after a clear code, one entry per code after the
    first, a wider code when the next free entry reaches 511 / 1023 / 2047 (``early=False``: 512 / 1024 / 2048)."""
    out, nbits, nxt, fresh = [], 9, FIRST, True
    for c in codes:
        out.append(nbits)
        if c == CLEAR:
            nbits, nxt, fresh = 9, FIRST, True
        elif c == EOI:
            pass
        elif fresh:
            fresh = False
        elif nxt < 4096:
            nxt += 1
            if nxt == (1 << nbits) - (1 if early else 0) and nbits < 12:
                nbits += 1
    return out


def pack(codes, *, early=True, lsb=False, code_widths=None) -> bytes:
    """The codes as bytes; the last byte padded with zeros."""
    acc = nbits_in = 0
    out = bytearray()
    for c, w in zip(codes, code_widths or widths(codes, early=early)):
        if lsb:
            acc |= c << nbits_in
            nbits_in += w
            while nbits_in >= 8:
                out.append(acc & 255)
                acc >>= 8
                nbits_in -= 8
        else:
            acc = (acc << w) | c
            nbits_in += w
            while nbits_in >= 8:
                out.append((acc >> (nbits_in - 8)) & 255)
                nbits_in -= 8
            acc &= (1 << nbits_in) - 1
    if nbits_in:
        out.append(acc & 255 if lsb else (acc << (8 - nbits_in)) & 255)
    return bytes(out)


def codes_of(data: bytes, *, clear_at=4094, open_clear=True, eoi=True, clear_every=None):
    """Greedy LZW codes of ``data``.  A clear code is sent when the READER's next free entry is ``clear_at`` (libtiff's writer:
    4094; 4096 = after the table's last entry; None = never), and after every ``clear_every`` codes."""
    out = [CLEAR] if open_clear else []
    table = {}
    nxt = FIRST                        # the reader's next free entry after the codes sent so far
    fresh = True
    w = b""
    since = 0
    for k in range(len(data)):
        c = data[k:k + 1]
        if len(w) == 0 or w + c in table:
            w = w + c
            continue
        out.append(table[w] if len(w) > 1 else w[0])
        since += 1
        if fresh:
            fresh = False
        elif nxt < 4096:
            nxt += 1
        if nxt + 1 <= 4096 and (FIRST + len(table)) < 4096:
            table[w + c] = FIRST + len(table)
        w = c
        if (clear_at is not None and nxt >= clear_at) or (clear_every and since >= clear_every):
            out.append(CLEAR)
            table, nxt, fresh, since = {}, FIRST, True, 0
    if w:
        out.append(table[w] if len(w) > 1 else w[0])
    if eoi:
        out.append(EOI)
    return out


def kwkwk_widths(codes):
    """The widths at which a code equal to the reader's next free entry (the KwKwK case) occurs."""
    seen, nxt, fresh = set(), FIRST, True
    for c, w in zip(codes, widths(codes)):
        if c == CLEAR:
            nxt, fresh = FIRST, True
        elif c == EOI:
            continue
        elif fresh:
            fresh = False
        else:
            if c == nxt:
                seen.add(w)
            if nxt < 4096:
                nxt += 1
    return seen


def lzw(data: bytes, **how) -> bytes:
    early = how.pop("early", True)
    return pack(codes_of(data, **how), early=early)


def packbits(data: bytes) -> bytes:
    """A plain PackBits encoder: runs of 3 or more as runs, the rest as literals."""
    out = bytearray()
    k, n = 0, len(data)
    while k < n:
        run = 1
        while k + run < n and run < 128 and data[k + run] == data[k]:
            run += 1
        if run >= 3:
            out += bytes([257 - run, data[k]])
            k += run
            continue
        lit = k
        while k < n and k - lit < 128:
            if k + 2 < n and data[k] == data[k + 1] == data[k + 2]:
                break
            k += 1
        out += bytes([k - lit - 1]) + data[lit:k]
    return bytes(out)
