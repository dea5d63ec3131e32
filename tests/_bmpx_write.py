"""A BMP writer for the files Pillow cannot write: exactly the header fields, palette, pixel bytes and RLE codes it is given (in
the manner of tests/_gif_write.py), the row packers of the 1-, 4- and 16-bit layouts, and a greedy RLE8 / RLE4 encoder on top for
real pictures."""
from __future__ import annotations

import struct

import numpy as np


def bmp(w, h, bits, data: bytes, *, hs=40, comp=0, colors=0, palette=b"", masks=(), offset=None, topdown=False, gap=0,
        height_field=None) -> bytes:
    """A BMP around pixel data given as it is.  masks: BITFIELDS -- inside the header for hs >= 52, behind it for hs == 40.
    offset: the data-offset field (default: where the data really starts); gap: bytes between palette and data."""
    height = height_field if height_field is not None else (-h if topdown else h)
    head = struct.pack("<iiHHIIiiII", w, height, 1, bits, comp, len(data), 2835, 2835, colors, 0)
    extra = b""
    if hs >= 52:
        m = list(masks) + [0] * (4 - len(masks))
        extra = struct.pack("<III", *m[:3]) + (struct.pack("<I", m[3]) if hs >= 56 else b"")
        extra += bytes(hs - 40 - len(extra))
    after = struct.pack("<III", *masks[:3]) if (hs == 40 and comp == 3) else b""
    body = struct.pack("<I", hs) + head + extra + after + palette + bytes(gap)
    off = 14 + len(body) if offset is None else offset
    return b"BM" + struct.pack("<IHHI", 14 + len(body) + len(data), 0, 0, off) + body + data


def data_start(hs=40, comp=0, ncolors=0, gap=0) -> int:
    """Where ``bmp`` puts the pixel data: what the parity of an absolute run's padding depends on."""
    return 14 + hs + (12 if hs == 40 and comp == 3 else 0) + 4 * ncolors + gap


def _stored(flat: np.ndarray, topdown: bool) -> bytes:
    pad = (-flat.shape[1]) % 4
    flat = np.concatenate([flat, np.zeros((flat.shape[0], pad), np.uint8)], 1)
    return (flat if topdown else flat[::-1]).tobytes()


def rows1(idx: np.ndarray, topdown=False) -> bytes:
    """H x W indices 0 / 1 -> stored rows, the most significant bit first, padded to four bytes."""
    return _stored(np.packbits(idx.astype(np.uint8) & 1, axis=1), topdown)


def rows4(idx: np.ndarray, topdown=False) -> bytes:
    """H x W indices 0 .. 15 -> stored rows, the high nibble first."""
    h, w = idx.shape
    a = np.zeros((h, w + (w & 1)), np.uint8)
    a[:, :w] = idx & 15
    return _stored((a[:, 0::2] << 4) | a[:, 1::2], topdown)


def rows16(px: np.ndarray, topdown=False) -> bytes:
    """H x W uint16 pixels -> stored rows, little endian."""
    h, w = px.shape
    return _stored(px.astype("<u2").view(np.uint8).reshape(h, 2 * w), topdown)


# ---- RLE codes, as bytes

EOL, EOB = b"\x00\x00", b"\x00\x01"


def run(n: int, v: int) -> bytes:
    assert 1 <= n <= 255
    return bytes([n, v])


def delta(right: int, up: int) -> bytes:
    return bytes([0, 2, right, up])


def absolute(n: int, payload: bytes, pad: bool = False) -> bytes:
    """(0, n) and the bytes given -- RLE8 wants n of them, RLE4 as Pillow reads it n // 2 --, then a padding byte if asked."""
    assert 3 <= n <= 255
    return bytes([0, n]) + payload + (b"\x00" if pad else b"")


class Stream:
    """RLE codes appended one by one; knows where in the file it stands, so ``absolute`` pads as Pillow's decoder skips: one
    byte when the position in the file behind the payload is odd."""

    def __init__(self, start: int, rle4: bool = False):
        self.start, self.rle4, self.b = start, rle4, bytearray()

    def add(self, code: bytes) -> "Stream":
        self.b += code
        return self

    def absolute(self, pixels) -> "Stream":
        n = len(pixels)
        if self.rle4:
            p = list(pixels) + [0]
            payload = bytes((p[k] << 4) | p[k + 1] for k in range(0, n - (n & 1), 2))      # n // 2 bytes: an odd n loses its last pixel
        else:
            payload = bytes(pixels)
        self.b += bytes([0, n]) + payload
        if (self.start + len(self.b)) & 1:
            self.b += b"\x00"
        return self

    def bytes(self) -> bytes:
        return bytes(self.b)


def encode_rle(idx: np.ndarray, start: int, rle4: bool = False, topdown: bool = False) -> bytes:
    """A greedy encoder: per stored row runs of three or more, everything between them as absolute runs (RLE4: of even length,
    since Pillow reads n // 2 bytes) or, where too short for one, runs of one or two; end-of-line behind every row but the
    last, end-of-bitmap behind that."""
    rows = idx if topdown else idx[::-1]
    s = Stream(start, rle4)
    for y, row in enumerate(rows.tolist()):
        w, x = len(row), 0
        lit: list = []

        def flush():
            nonlocal lit
            while lit:
                take = min(len(lit), 254)
                if rle4:
                    take -= take & 1
                if take >= 3:
                    s.absolute(lit[:take])
                else:
                    take = min(len(lit), 2)
                    s.add(run(take, (lit[0] << 4 | (lit[1] if take == 2 else 0)) if rle4 else lit[0]) if rle4 or take == 1 or lit[0] == lit[1]
                          else run(1, lit[0]) + run(1, lit[1]))
                lit = lit[take:]

        while x < w:
            if rle4:
                a, b = row[x], row[x + 1] if x + 1 < w else row[x]
                n = 1
                while x + n < w and n < 255 and row[x + n] == (b if n & 1 else a):
                    n += 1
                value = (a << 4) | b
            else:
                n = 1
                while x + n < w and n < 255 and row[x + n] == row[x]:
                    n += 1
                value = row[x]
            if n >= 3:
                flush()
                s.add(run(n, value))
                x += n
            else:
                lit.append(row[x])
                x += 1
        flush()
        s.add(EOL if y + 1 < len(rows) else EOB)
    return s.bytes()
