"""A VP8 partition-0 rewriter for the lossy WebP decoder's tests (RFC 6386).

A key frame keeps its whole frame header and every macroblock's modes in partition 0, and the residual tokens in separate
partitions.  parse() decodes partition 0 into values; emit() encodes it again, with whatever header fields and modes the
caller set, and copies the token partitions byte for byte.  What the tokens depend on has to stay: every macroblock's
is_i4 and skip flag, the partition count and the coefficient-probability updates.  The rest is free, so files can carry
headers and modes no encoder chooses to write, and Pillow (libwebp) decoding the rewritten bytes stays the reference.

The second half builds the rewritten corpora the CPU and GPU tests share (modes, filter, header bits, quant-down,
quant-up), each from a seed, on bases Pillow encodes and on the committed files under tests/golden/webp/."""
from __future__ import annotations

import copy
import struct

import numpy as np

import _webp_cases as W

# ---- spec tables (RFC 6386): coefficient update probabilities (13.4), key-frame sub-block mode probabilities (11.5) ---------
COEFF_UPDATE_PROBA = bytes([  # 1056
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 176, 246, 255, 255, 255, 255, 255, 255, 255, 255, 255, 223, 241,
    252, 255, 255, 255, 255, 255, 255, 255, 255, 249, 253, 253, 255, 255, 255, 255, 255, 255, 255, 255, 255, 244, 252,
    255, 255, 255, 255, 255, 255, 255, 255, 234, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 253, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 246, 254, 255, 255, 255, 255, 255, 255, 255, 255, 239, 253, 254, 255, 255,
    255, 255, 255, 255, 255, 255, 254, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 248, 254, 255, 255, 255,
    255, 255, 255, 255, 255, 251, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 251, 254, 254, 255, 255, 255, 255, 255,
    255, 255, 255, 254, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 253, 255, 254, 255, 255, 255, 255,
    255, 255, 250, 255, 254, 255, 254, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 217, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 225,
    252, 241, 253, 255, 255, 254, 255, 255, 255, 255, 234, 250, 241, 250, 253, 255, 253, 254, 255, 255, 255, 255, 254,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 223, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 238, 253, 254,
    254, 255, 255, 255, 255, 255, 255, 255, 255, 248, 254, 255, 255, 255, 255, 255, 255, 255, 255, 249, 254, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 253, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 247, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 252, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 254, 255, 255, 255, 255, 255,
    255, 255, 255, 253, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 254, 253, 255, 255, 255, 255, 255, 255, 255, 255, 250, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 186,
    251, 250, 255, 255, 255, 255, 255, 255, 255, 255, 234, 251, 244, 254, 255, 255, 255, 255, 255, 255, 255, 251, 251,
    243, 253, 254, 255, 254, 255, 255, 255, 255, 255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 236, 253, 254,
    255, 255, 255, 255, 255, 255, 255, 255, 251, 253, 253, 254, 254, 255, 255, 255, 255, 255, 255, 255, 254, 254, 255,
    255, 255, 255, 255, 255, 255, 255, 254, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 254, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 248, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 250, 254,
    252, 254, 255, 255, 255, 255, 255, 255, 255, 248, 254, 249, 253, 255, 255, 255, 255, 255, 255, 255, 255, 253, 253,
    255, 255, 255, 255, 255, 255, 255, 255, 246, 253, 253, 255, 255, 255, 255, 255, 255, 255, 255, 252, 254, 251, 254,
    254, 255, 255, 255, 255, 255, 255, 255, 254, 252, 255, 255, 255, 255, 255, 255, 255, 255, 248, 254, 253, 255, 255,
    255, 255, 255, 255, 255, 255, 253, 255, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 251, 254, 255, 255, 255,
    255, 255, 255, 255, 255, 245, 251, 254, 255, 255, 255, 255, 255, 255, 255, 255, 253, 253, 254, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 251, 253, 255, 255, 255, 255, 255, 255, 255, 255, 252, 253, 254, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 252, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 249, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 253, 255, 255, 255, 255, 255, 255, 255, 255, 250, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255
])
BMODES_PROBA = bytes([  # 900
    231, 120, 48, 89, 115, 113, 120, 152, 112, 152, 179, 64, 126, 170, 118, 46, 70, 95, 175, 69, 143, 80, 85, 82, 72,
    155, 103, 56, 58, 10, 171, 218, 189, 17, 13, 152, 114, 26, 17, 163, 44, 195, 21, 10, 173, 121, 24, 80, 195, 26, 62,
    44, 64, 85, 144, 71, 10, 38, 171, 213, 144, 34, 26, 170, 46, 55, 19, 136, 160, 33, 206, 71, 63, 20, 8, 114, 114,
    208, 12, 9, 226, 81, 40, 11, 96, 182, 84, 29, 16, 36, 134, 183, 89, 137, 98, 101, 106, 165, 148, 72, 187, 100, 130,
    157, 111, 32, 75, 80, 66, 102, 167, 99, 74, 62, 40, 234, 128, 41, 53, 9, 178, 241, 141, 26, 8, 107, 74, 43, 26, 146,
    73, 166, 49, 23, 157, 65, 38, 105, 160, 51, 52, 31, 115, 128, 104, 79, 12, 27, 217, 255, 87, 17, 7, 87, 68, 71, 44,
    114, 51, 15, 186, 23, 47, 41, 14, 110, 182, 183, 21, 17, 194, 66, 45, 25, 102, 197, 189, 23, 18, 22, 88, 88, 147,
    150, 42, 46, 45, 196, 205, 43, 97, 183, 117, 85, 38, 35, 179, 61, 39, 53, 200, 87, 26, 21, 43, 232, 171, 56, 34, 51,
    104, 114, 102, 29, 93, 77, 39, 28, 85, 171, 58, 165, 90, 98, 64, 34, 22, 116, 206, 23, 34, 43, 166, 73, 107, 54, 32,
    26, 51, 1, 81, 43, 31, 68, 25, 106, 22, 64, 171, 36, 225, 114, 34, 19, 21, 102, 132, 188, 16, 76, 124, 62, 18, 78,
    95, 85, 57, 50, 48, 51, 193, 101, 35, 159, 215, 111, 89, 46, 111, 60, 148, 31, 172, 219, 228, 21, 18, 111, 112, 113,
    77, 85, 179, 255, 38, 120, 114, 40, 42, 1, 196, 245, 209, 10, 25, 109, 88, 43, 29, 140, 166, 213, 37, 43, 154, 61,
    63, 30, 155, 67, 45, 68, 1, 209, 100, 80, 8, 43, 154, 1, 51, 26, 71, 142, 78, 78, 16, 255, 128, 34, 197, 171, 41,
    40, 5, 102, 211, 183, 4, 1, 221, 51, 50, 17, 168, 209, 192, 23, 25, 82, 138, 31, 36, 171, 27, 166, 38, 44, 229, 67,
    87, 58, 169, 82, 115, 26, 59, 179, 63, 59, 90, 180, 59, 166, 93, 73, 154, 40, 40, 21, 116, 143, 209, 34, 39, 175,
    47, 15, 16, 183, 34, 223, 49, 45, 183, 46, 17, 33, 183, 6, 98, 15, 32, 183, 57, 46, 22, 24, 128, 1, 54, 17, 37, 65,
    32, 73, 115, 28, 128, 23, 128, 205, 40, 3, 9, 115, 51, 192, 18, 6, 223, 87, 37, 9, 115, 59, 77, 64, 21, 47, 104, 55,
    44, 218, 9, 54, 53, 130, 226, 64, 90, 70, 205, 40, 41, 23, 26, 57, 54, 57, 112, 184, 5, 41, 38, 166, 213, 30, 34,
    26, 133, 152, 116, 10, 32, 134, 39, 19, 53, 221, 26, 114, 32, 73, 255, 31, 9, 65, 234, 2, 15, 1, 118, 73, 75, 32,
    12, 51, 192, 255, 160, 43, 51, 88, 31, 35, 67, 102, 85, 55, 186, 85, 56, 21, 23, 111, 59, 205, 45, 37, 192, 55, 38,
    70, 124, 73, 102, 1, 34, 98, 125, 98, 42, 88, 104, 85, 117, 175, 82, 95, 84, 53, 89, 128, 100, 113, 101, 45, 75, 79,
    123, 47, 51, 128, 81, 171, 1, 57, 17, 5, 71, 102, 57, 53, 41, 49, 38, 33, 13, 121, 57, 73, 26, 1, 85, 41, 10, 67,
    138, 77, 110, 90, 47, 114, 115, 21, 2, 10, 102, 255, 166, 23, 6, 101, 29, 16, 10, 85, 128, 101, 196, 26, 57, 18, 10,
    102, 102, 213, 34, 20, 43, 117, 20, 15, 36, 163, 128, 68, 1, 26, 102, 61, 71, 37, 34, 53, 31, 243, 192, 69, 60, 71,
    38, 73, 119, 28, 222, 37, 68, 45, 128, 34, 1, 47, 11, 245, 171, 62, 17, 19, 70, 146, 85, 55, 62, 70, 37, 43, 37,
    154, 100, 163, 85, 160, 1, 63, 9, 92, 136, 28, 64, 32, 201, 85, 75, 15, 9, 9, 64, 255, 184, 119, 16, 86, 6, 28, 5,
    64, 255, 25, 248, 1, 56, 8, 17, 132, 137, 255, 55, 116, 128, 58, 15, 20, 82, 135, 57, 26, 121, 40, 164, 50, 31, 137,
    154, 133, 25, 35, 218, 51, 103, 44, 131, 131, 123, 31, 6, 158, 86, 40, 64, 135, 148, 224, 45, 183, 128, 22, 26, 17,
    131, 240, 154, 14, 1, 209, 45, 16, 21, 91, 64, 222, 7, 1, 197, 56, 21, 39, 155, 60, 138, 23, 102, 213, 83, 12, 13,
    54, 192, 255, 68, 47, 28, 85, 26, 85, 85, 128, 128, 32, 146, 171, 18, 11, 7, 63, 144, 171, 4, 4, 246, 35, 27, 10,
    146, 174, 171, 12, 26, 128, 190, 80, 35, 99, 180, 80, 126, 54, 45, 85, 126, 47, 87, 176, 51, 41, 20, 32, 101, 75,
    128, 139, 118, 146, 116, 128, 85, 56, 41, 15, 176, 236, 85, 37, 9, 62, 71, 30, 17, 119, 118, 255, 17, 18, 138, 101,
    38, 60, 138, 55, 70, 43, 26, 142, 146, 36, 19, 30, 171, 255, 97, 27, 20, 138, 45, 61, 62, 219, 1, 81, 188, 64, 32,
    41, 20, 117, 151, 142, 20, 21, 163, 112, 19, 12, 61, 195, 128, 48, 4, 24
])

# modes numbered as the decoder numbers them; DC / TM / V / H are also the 16x16 and chroma modes
B_DC, B_TM, B_VE, B_HE, B_RD, B_VR, B_LD, B_VL, B_HD, B_HU = range(10)
BMODE_NAMES = ("DC", "TM", "V", "H", "RD", "VR", "LD", "VL", "HD", "HU")
# sub-block mode tree (section 11.2): node i has entries [2 i], [2 i + 1]; a positive entry is the next node, -entry a leaf
_BTREE = (-B_DC, 1, -B_TM, 2, -B_VE, 3, 4, 6, -B_HE, 5, -B_RD, -B_VR, -B_LD, 7, -B_VL, 8, -B_HD, -B_HU)


def _tree_paths(tree) -> dict:
    """leaf -> [(node, bit)] from the root"""
    out = {}

    def walk(node, path):
        for bit in (0, 1):
            e = tree[2 * node + bit]
            if e > 0:
                walk(e, path + [(node, bit)])
            else:
                out[-e] = path + [(node, bit)]

    walk(0, [])
    return out


_BPATH = _tree_paths(_BTREE)
# 16x16 and chroma trees of a key frame (section 11.2, 11.4): mode -> [(prob, bit)]
_YPATH = {B_DC: ((156, 0), (163, 0)), B_VE: ((156, 0), (163, 1)), B_HE: ((156, 1), (128, 0)), B_TM: ((156, 1), (128, 1))}
_UVPATH = {B_DC: ((142, 0),), B_VE: ((142, 1), (114, 0)), B_TM: ((142, 1), (114, 1), (183, 1)),
           B_HE: ((142, 1), (114, 1), (183, 0))}


# ---- boolean decoder and encoder (section 7.3) -----------------------------------------------------------------------------
class BoolDecoder:
    """Reads past the end as zero bytes."""

    def __init__(self, data: bytes):
        self.data, self.pos = data, 2
        self.value = (data[0] << 8 if len(data) > 0 else 0) | (data[1] if len(data) > 1 else 0)
        self.range, self.count = 255, 0

    def bit(self, prob: int) -> int:
        split = 1 + (((self.range - 1) * prob) >> 8)
        big = split << 8
        if self.value >= big:
            b, self.range, self.value = 1, self.range - split, self.value - big
        else:
            b, self.range = 0, split
        while self.range < 128:
            self.value <<= 1
            self.range <<= 1
            self.count += 1
            if self.count == 8:
                self.count = 0
                if self.pos < len(self.data):
                    self.value |= self.data[self.pos]
                self.pos += 1
        return b

    def literal(self, n: int) -> int:
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit(128)
        return v

    def optional_signed(self, n: int):
        """a flag, then magnitude and sign: None when the flag is off"""
        if not self.bit(128):
            return None
        v = self.literal(n)
        return -v if self.bit(128) else v


class BoolEncoder:
    def __init__(self):
        self.out = bytearray()
        self.range, self.bottom, self.count = 255, 0, 24

    def _carry(self):
        k = len(self.out) - 1
        while k >= 0 and self.out[k] == 255:
            self.out[k] = 0
            k -= 1
        self.out[k] += 1

    def bit(self, prob: int, b: int) -> None:
        split = 1 + (((self.range - 1) * prob) >> 8)
        if b:
            self.bottom += split
            self.range -= split
        else:
            self.range = split
        while self.range < 128:
            self.range <<= 1
            if self.bottom & (1 << 31):
                self._carry()
            self.bottom = (self.bottom << 1) & 0xFFFFFFFF
            self.count -= 1
            if self.count == 0:
                self.out.append(self.bottom >> 24)
                self.bottom &= (1 << 24) - 1
                self.count = 8

    def literal(self, v: int, n: int) -> None:
        for k in range(n - 1, -1, -1):
            self.bit(128, (v >> k) & 1)

    def optional_signed(self, v, n: int) -> None:
        self.bit(128, v is not None)
        if v is not None:
            assert abs(v) < (1 << n), (v, n)
            self.literal(abs(v), n)
            self.bit(128, v < 0)

    def finish(self) -> bytes:
        for _ in range(32):                                  # pushes every pending bit out (libvpx's stop_encode)
            self.bit(128, 0)
        return bytes(self.out)


# ---- parse / emit ----------------------------------------------------------------------------------------------------------
class Frame:
    """One key frame as values.  Optional header values are None where their flag is off.  mbs: one dict per macroblock in
    raster order with segment, skip, is_i4, ymode (16x16, None for B_PRED), bmodes (16 sub-block modes, None otherwise),
    uvmode."""

    def __repr__(self):
        shown = (f"{k}={v!r}" for k, v in vars(self).items() if k not in ("mbs", "coeff_updates", "tail"))
        return "Frame(" + ", ".join(shown) + ")"


def parse(data: bytes) -> Frame:
    chunks = dict(W.chunks(data))
    vp8 = chunks[b"VP8 "]
    f = Frame()
    f.container = "vp8x" if b"VP8X" in chunks else "simple"
    tag = vp8[0] | vp8[1] << 8 | vp8[2] << 16
    assert not tag & 1 and (tag >> 4) & 1 and vp8[3:6] == b"\x9d\x01\x2a", "not a shown key frame"
    f.profile, part0 = (tag >> 1) & 7, tag >> 5
    wb, hb = struct.unpack("<HH", vp8[6:10])
    f.width, f.height, f.xscale, f.yscale = wb & 0x3FFF, hb & 0x3FFF, wb >> 14, hb >> 14
    f.mb_w, f.mb_h = (f.width + 15) >> 4, (f.height + 15) >> 4
    f.tail = vp8[10 + part0:]
    br = BoolDecoder(vp8[10:10 + part0])
    f.color_space, f.clamping = br.literal(1), br.literal(1)
    f.use_segment = br.literal(1)
    f.update_map = f.update_data = 0
    f.absolute, f.seg_quant, f.seg_lf, f.seg_probs = 1, [None] * 4, [None] * 4, [None] * 3
    if f.use_segment:
        f.update_map, f.update_data = br.literal(1), br.literal(1)
        if f.update_data:
            f.absolute = br.literal(1)
            f.seg_quant = [br.optional_signed(7) for _ in range(4)]
            f.seg_lf = [br.optional_signed(6) for _ in range(4)]
        if f.update_map:
            f.seg_probs = [br.literal(8) if br.bit(128) else None for _ in range(3)]
    f.simple, f.level, f.sharpness = br.literal(1), br.literal(6), br.literal(3)
    f.use_lf_delta, f.lf_update, f.ref_lf, f.mode_lf = br.literal(1), 0, [None] * 4, [None] * 4
    if f.use_lf_delta:
        f.lf_update = br.literal(1)
        if f.lf_update:
            f.ref_lf = [br.optional_signed(6) for _ in range(4)]
            f.mode_lf = [br.optional_signed(6) for _ in range(4)]
    f.log2_parts = br.literal(2)
    f.base_q = br.literal(7)
    f.dq = [br.optional_signed(4) for _ in range(5)]            # Y1 DC, Y2 DC, Y2 AC, UV DC, UV AC
    f.refresh_entropy = br.literal(1)
    f.coeff_updates = [br.literal(8) if br.bit(p) else None for p in COEFF_UPDATE_PROBA]
    f.use_skip = br.literal(1)
    f.skip_p = br.literal(8) if f.use_skip else None
    probs = [255 if p is None else p for p in f.seg_probs]
    top = [0] * (4 * f.mb_w)
    f.mbs = []
    for y in range(f.mb_h):
        left = [0] * 4
        for x in range(f.mb_w):
            m = {"segment": 0, "skip": 0}
            if f.update_map:
                m["segment"] = br.bit(probs[1]) if not br.bit(probs[0]) else 2 + br.bit(probs[2])
            if f.use_skip:
                m["skip"] = br.bit(f.skip_p)
            m["is_i4"] = not br.bit(145)
            t = top[4 * x:4 * x + 4]
            if not m["is_i4"]:
                ym = (B_TM if br.bit(128) else B_HE) if br.bit(156) else (B_VE if br.bit(163) else B_DC)
                m["ymode"], m["bmodes"] = ym, None
                t, left = [ym] * 4, [ym] * 4
            else:
                bm = [0] * 16
                for by in range(4):
                    for bx in range(4):
                        prob = BMODES_PROBA[90 * t[bx] + 9 * left[by]:][:9]
                        i = _BTREE[br.bit(prob[0])]
                        while i > 0:
                            i = _BTREE[2 * i + br.bit(prob[i])]
                        bm[4 * by + bx] = t[bx] = left[by] = -i
                m["ymode"], m["bmodes"] = None, bm
            top[4 * x:4 * x + 4] = t
            m["uvmode"] = B_DC if not br.bit(142) else B_VE if not br.bit(114) else B_TM if br.bit(183) else B_HE
            f.mbs.append(m)
    return f


def _partition0(f: Frame) -> bytes:
    e = BoolEncoder()
    e.literal(f.color_space, 1)
    e.literal(f.clamping, 1)
    e.literal(f.use_segment, 1)
    if f.use_segment:
        e.literal(f.update_map, 1)
        e.literal(f.update_data, 1)
        if f.update_data:
            e.literal(f.absolute, 1)
            for v in f.seg_quant:
                e.optional_signed(v, 7)
            for v in f.seg_lf:
                e.optional_signed(v, 6)
        if f.update_map:
            for v in f.seg_probs:
                e.bit(128, v is not None)
                if v is not None:
                    e.literal(v, 8)
    e.literal(f.simple, 1)
    e.literal(f.level, 6)
    e.literal(f.sharpness, 3)
    e.literal(f.use_lf_delta, 1)
    if f.use_lf_delta:
        e.literal(f.lf_update, 1)
        if f.lf_update:
            for v in f.ref_lf + f.mode_lf:
                e.optional_signed(v, 6)
    e.literal(f.log2_parts, 2)
    e.literal(f.base_q, 7)
    for v in f.dq:
        e.optional_signed(v, 4)
    e.literal(f.refresh_entropy, 1)
    for p, v in zip(COEFF_UPDATE_PROBA, f.coeff_updates):
        e.bit(p, v is not None)
        if v is not None:
            e.literal(v, 8)
    e.literal(f.use_skip, 1)
    if f.use_skip:
        e.literal(f.skip_p, 8)
    probs = [255 if p is None else p for p in f.seg_probs]
    top = [0] * (4 * f.mb_w)
    for y in range(f.mb_h):
        left = [0] * 4
        for x in range(f.mb_w):
            m = f.mbs[y * f.mb_w + x]
            if f.update_map:
                s = m["segment"]
                e.bit(probs[0], s >= 2)
                e.bit(probs[1 + (s >= 2)], s & 1)
            if f.use_skip:
                e.bit(f.skip_p, m["skip"])
            else:
                assert not m["skip"], "a skipped macroblock needs use_skip"
            e.bit(145, not m["is_i4"])
            t = top[4 * x:4 * x + 4]
            if not m["is_i4"]:
                for p, b in _YPATH[m["ymode"]]:
                    e.bit(p, b)
                t, left = [m["ymode"]] * 4, [m["ymode"]] * 4
            else:
                for by in range(4):
                    for bx in range(4):
                        mode = m["bmodes"][4 * by + bx]
                        prob = BMODES_PROBA[90 * t[bx] + 9 * left[by]:][:9]
                        for node, b in _BPATH[mode]:
                            e.bit(prob[node], b)
                        t[bx] = left[by] = mode
            top[4 * x:4 * x + 4] = t
            for p, b in _UVPATH[m["uvmode"]]:
                e.bit(p, b)
    return e.finish()


def emit(f: Frame, container: str = "simple") -> bytes:
    """The file of frame f: partition 0 encoded again, the token partitions (size table and data) copied unchanged."""
    p0 = _partition0(f)
    assert len(p0) < 1 << 19
    tag = (f.profile << 1) | (1 << 4) | (len(p0) << 5)
    vp8 = (bytes([tag & 255, (tag >> 8) & 255, tag >> 16]) + b"\x9d\x01\x2a"
           + struct.pack("<HH", f.width | f.xscale << 14, f.height | f.yscale << 14) + p0 + f.tail)
    if container == "vp8x":
        return W.vp8x(vp8, canvas=(f.width, f.height))
    assert container == "simple"
    return W.riff([(b"VP8 ", vp8)])


# ---- what a frame's header makes of its segments (libwebp's VP8ParseQuant / PrecomputeFilterStrengths) -------------------
def _clip(v: int, m: int) -> int:
    return 0 if v < 0 else m if v > m else v


def segment_q(f: Frame, s: int) -> int:
    """the quantiser index of segment s before the deltas"""
    if not f.use_segment:
        return f.base_q
    q = f.seg_quant[s] or 0
    return q if f.absolute else q + f.base_q


def quant_indices(f: Frame, s: int) -> tuple:
    """the six effective indices of segment s: Y1 DC, Y1 AC, Y2 DC, Y2 AC, UV DC, UV AC"""
    q, d = segment_q(f, s), [v or 0 for v in f.dq]
    return (_clip(q + d[0], 127), _clip(q, 127), _clip(q + d[1], 127), _clip(q + d[2], 127), _clip(q + d[3], 117),
            _clip(q + d[4], 127))


def filter_level(f: Frame, s: int, i4: bool) -> int:
    """the effective loop-filter level of segment s for 16x16 (i4 False) or B_PRED macroblocks; 0: none"""
    if f.level == 0:
        return 0                                             # libwebp turns the filter off for the frame
    lv = f.level
    if f.use_segment:
        lv = f.seg_lf[s] or 0
        if not f.absolute:
            lv += f.level
    if f.use_lf_delta:
        lv += f.ref_lf[0] or 0
        if i4:
            lv += f.mode_lf[0] or 0
    return _clip(lv, 63)


def position_classes(f: Frame, x: int, y: int) -> list:
    """corner / top / left / right / interior, and partial for the last row / column of a frame whose side is not a
    multiple of 16"""
    out = ["corner" if x == 0 and y == 0 else "top" if y == 0 else "left" if x == 0 else
           "right" if x == f.mb_w - 1 else "interior"]
    if x == f.mb_w - 1 and y > 0 and out[0] != "right":
        out.append("right")
    if (y == f.mb_h - 1 and f.height % 16) or (x == f.mb_w - 1 and f.width % 16):
        out.append("partial")
    return out


POSITIONS = ("corner", "top", "left", "right", "interior", "partial")


def mb_indices(f: Frame) -> list:
    """the six effective quantiser indices of every macroblock"""
    per = [quant_indices(f, s) for s in range(4)]
    return [per[m["segment"]] for m in f.mbs]


def dequant_never_grows(base: Frame, new: Frame) -> bool:
    """Every macroblock's six indices at most the base's, and the Y2 ones equal where the macroblock has a Y2 block: no
    dequantised value can grow (the steps rise with the index), so the decoder's coefficient limit is not crossed."""
    for m, a, b in zip(base.mbs, mb_indices(base), mb_indices(new)):
        if any(y > x for x, y in zip(a, b)) or (not m["is_i4"] and a[2:4] != b[2:4]):
            return False
    return True


# ---- bases -----------------------------------------------------------------------------------------------------------------
# 1x1, 1xN, Nx1, 15 / 16 / 17 and 31 / 32 / 33 on each side, and a frame of 65 macroblocks per row
BASE_SIZES = ((1, 1), (1, 40), (40, 1), (15, 15), (16, 16), (17, 17), (31, 31), (32, 32), (33, 33), (15, 33), (33, 15),
              (16, 31), (31, 16), (17, 32), (32, 17), (47, 50), (1040, 17))


def pillow_bases(seed: int, kinds=W.KINDS, quality=(30, 96), sizes=BASE_SIZES) -> list:
    """[(name, bytes)] Pillow writes at the sizes above"""
    rng = np.random.default_rng(seed)
    out = []
    for i, (w, h) in enumerate(sizes):
        kind, q = kinds[i % len(kinds)], int(rng.integers(*quality))
        out.append((f"{kind}_{w}x{h}_q{q}", W.pillow_file(W.content(rng, w, h, kind), q, int(rng.integers(0, 7)))))
    return out


def _bases(seed: int, golden_every: int = 2, **kw) -> list:
    return pillow_bases(seed, **kw) + W.golden_cases()[::golden_every]


# ---- what the groups change --------------------------------------------------------------------------------------------------
def random_modes(f: Frame, rng, k: int = 0) -> str:
    for m in f.mbs:
        if m["is_i4"]:
            m["bmodes"] = [int(v) for v in rng.integers(0, 10, 16)]
        else:
            m["ymode"] = int(rng.integers(0, 4))
        m["uvmode"] = int(rng.integers(0, 4))
    return "simple"


def _segments_free(f: Frame, rng, absolute: int) -> None:
    """Segmentation on with a map and a data update, every macroblock's quantiser kept: a base without segments gets random
    ids over four equal segments; a base with them keeps its ids and segment quantisers (in either mode)."""
    qs = [segment_q(f, s) for s in range(4)]
    if not f.use_segment:
        for m in f.mbs:
            m["segment"] = int(rng.integers(0, 4))
    elif not f.update_map:
        qs = [qs[0]] * 4
    f.use_segment = f.update_map = f.update_data = 1
    f.absolute = absolute
    f.seg_quant = [q if absolute else q - f.base_q for q in qs]
    if f.seg_probs == [None] * 3:
        f.seg_probs = [int(v) for v in rng.integers(1, 255, 3)]


FILTER_LEVELS = (0, 1, 14, 15, 16, 39, 40, 41, 63)


def filter_variant(f: Frame, rng, k: int) -> str:
    """Simple or normal filter, sharpness 0-7, per-segment levels taking FILTER_LEVELS in turn (absolute or relative to the
    frame's), loop-filter deltas on every other variant with values that can push a level under 0 or over 63, and frame
    level 0 with non-zero segment strengths every ninth."""
    f.simple, f.sharpness = k % 2, int(rng.integers(0, 8))
    absolute = int(rng.integers(0, 2))
    _segments_free(f, rng, absolute)
    f.level = int(rng.integers(1, 64))
    f.use_lf_delta = f.lf_update = 0
    ref = 0
    if k % 2 == 1 and k % 9 != 8:
        f.use_lf_delta = 1
        f.lf_update = int(k % 4 != 3)            # deltas on without an update: all zero
        if f.lf_update:
            f.ref_lf = [int(v) if v else None for v in rng.integers(-63, 64, 4)]
            f.mode_lf = [int(v) if v else None for v in rng.integers(-63, 64, 4)]
            f.ref_lf[0] = int(rng.integers(-12, 13))
            f.mode_lf[0] = int(rng.choice([-63, -40, -15, -1, 1, 15, 25, 40, 63]))
            ref = f.ref_lf[0]
    targets = [FILTER_LEVELS[(4 * k + s) % len(FILTER_LEVELS)] for s in range(4)]
    seg = [max(-63, min(63, t - ref)) for t in targets]
    f.seg_lf = [v if absolute else max(-63, min(63, v - f.level)) for v in seg]
    if k % 9 == 8:
        f.level = 0                                   # the frame's level 0 turns the filter off, whatever the segments say
        f.seg_lf = [int(v) for v in rng.integers(1, 64, 4)]
    return "simple"


def header_variant(f: Frame, rng, k: int) -> str:
    """Profile, scale bits, colour space and clamping bits, segmentation without a map update, segment-tree probabilities,
    skip probability; returns the container."""
    f.profile = k % 4
    f.xscale, f.yscale = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    f.color_space, f.clamping = int(rng.integers(0, 2)), int(rng.integers(0, 2))
    f.refresh_entropy = int(rng.integers(0, 2))
    what = k % 3
    per_mb = set(mb_indices(f))
    if what == 0 and len(per_mb) == 1:                # segmentation without a map: every macroblock in segment 0
        q = segment_q(f, f.mbs[0]["segment"])
        absolute = int(rng.integers(0, 2))
        f.use_segment, f.update_map, f.update_data, f.absolute = 1, 0, 1, absolute
        f.seg_quant = [q if absolute else q - f.base_q] + [int(v) for v in rng.integers(-127, 128, 3)]
        f.seg_lf = [int(v) if v else None for v in rng.integers(-63, 64, 4)]
        f.seg_probs = [None] * 3
        for m in f.mbs:
            m["segment"] = 0
    elif what == 1:                                   # segment-tree probabilities, 0 and 255 among them
        _segments_free(f, rng, int(rng.integers(0, 2)))
        f.seg_probs = [int(rng.choice([0, 255, int(rng.integers(1, 255))])) if rng.integers(0, 4) else None for _ in range(3)]
        f.seg_probs[k % 3] = (0, 255, None)[(k // 3) % 3]
    if f.use_skip and not any(m["skip"] for m in f.mbs) and rng.integers(0, 2):
        f.use_skip, f.skip_p = 0, None
    elif f.use_skip or rng.integers(0, 2):
        f.use_skip, f.skip_p = 1, int(rng.choice([0, 255, int(rng.integers(1, 255))]))
    return "vp8x" if k % 2 else "simple"


def quant_down_variant(f: Frame, rng, k: int):
    """Per-segment quantisers and Y1 DC / UV deltas, absolute or relative, no index above the base's and the Y2 indices
    kept through the Y2 deltas; every fourth draw on a base whose Y2 indices allow it: segmentation without a data update
    (every segment at q = 0).  False when the draw cannot keep that rule."""
    base = copy.deepcopy(f)
    old = mb_indices(base)
    y2 = {old[i][2:4] for i, m in enumerate(base.mbs) if not m["is_i4"]}
    if k % 4 == 3 and len(y2) <= 1 and all(v <= 15 for t in y2 for v in t):
        dc, ac = next(iter(y2)) if y2 else (int(rng.integers(0, 16)), int(rng.integers(0, 16)))
        f.use_segment, f.update_data, f.absolute = 1, 0, 1
        f.seg_quant, f.seg_lf = [None] * 4, [None] * 4
        if not base.use_segment:
            f.update_map = int(rng.integers(0, 2))
            for m in f.mbs:
                m["segment"] = int(rng.integers(0, 4)) if f.update_map else 0
            if f.update_map:
                f.seg_probs = [int(v) for v in rng.integers(0, 256, 3)]
        f.base_q = int(rng.integers(0, 128))       # not used: every segment is at 0
        y1dc, uvdc, uvac = (min(o[j] for o in old) for j in (0, 4, 5))
        f.dq = [int(rng.integers(-15, min(15, y1dc) + 1)), dc, ac, int(rng.integers(-15, min(15, uvdc) + 1)),
                int(rng.integers(-15, min(15, uvac) + 1))]
    else:
        if not base.use_segment:                     # segments 0 / 1 hold the 16x16 macroblocks, 2 / 3 only B_PRED ones
            f.use_segment, f.update_map, f.update_data = 1, 1, 1
            f.seg_probs = [int(v) for v in rng.integers(0, 256, 3)]
            for m in f.mbs:
                m["segment"] = int(rng.integers(0, 4 if m["is_i4"] else 2))
            qs = [base.base_q] * 4
        else:
            f.update_data = 1
            qs = [segment_q(base, s) for s in range(4)]
        i16 = {m["segment"] for m in f.mbs if not m["is_i4"]}
        d = int(rng.integers(-15, 1))
        new_q = [q + d if s in i16 or not rng.integers(0, 3) else q - int(rng.integers(0, q + 12)) for s, q in enumerate(qs)]
        d2 = [v or 0 for v in base.dq]
        if abs(d2[1] - d) > 15 or abs(d2[2] - d) > 15:
            return False
        f.dq = [None] * 5
        f.dq[1], f.dq[2] = d2[1] - d, d2[2] - d
        for j, col in ((0, 0), (3, 4), (4, 5)):
            cap = min([o[col] - new_q[m["segment"]] for o, m in zip(old, f.mbs)] + [15])
            f.dq[j] = int(rng.integers(-15, max(-15, cap) + 1))
        f.absolute = int(rng.integers(0, 2))
        if f.absolute:                              # the frame's index is then unused: 0 and 127 among the draws
            f.base_q = int(rng.choice([0, 127, int(rng.integers(0, 128))]))
        else:
            f.base_q = max(0, min(127, new_q[0] + int(rng.integers(-20, 21))))
        f.seg_quant = [q if f.absolute else q - f.base_q for q in new_q]
        if any(abs(v) > 127 for v in f.seg_quant):
            return False
    f.dq = [v if v or rng.integers(0, 2) else None for v in f.dq]
    return "simple" if dequant_never_grows(base, f) else False


def quant_up_variant(f: Frame, rng, k: int) -> str:
    """Indices from the base's up to 127, deltas up to +-15: the draws that can cross the decoder's coefficient limit."""
    qs = [segment_q(f, s) for s in range(4)]
    top = (qs[0] + 6, qs[0] + 30, 127)[k % 3]
    if not f.use_segment:
        f.update_map = 0
    f.use_segment, f.update_data, f.absolute = 1, 1, int(rng.integers(0, 2))
    if not f.update_map:
        qs = [qs[0]] * 4
    new_q = [int(rng.integers(q, max(q, min(127, top)) + 1)) for q in qs]
    if k % 6 == 2:
        new_q = [127] * 4
    f.base_q = int(rng.integers(0, 128)) if f.absolute else int(rng.integers(max(0, max(new_q) - 127), min(new_q) + 1))
    f.seg_quant = [q if f.absolute else q - f.base_q for q in new_q]
    f.dq = [int(v) if v else None for v in rng.integers(-15, 16, 5)]
    return "simple"


# ---- the corpora: [(name, bytes, the intended Frame)] ------------------------------------------------------------------------
def _group(bases, rng, variant, per: int, tag: str) -> list:
    """per draws of variant(frame, rng, k) on each base: it changes the frame in place and returns the container, or False
    to drop the draw"""
    out = []
    for bname, data in bases:
        base = parse(data)
        for _ in range(per):
            f = copy.deepcopy(base)
            container = variant(f, rng, len(out))
            if container:
                out.append((f"{tag}_{len(out)}_{bname}", emit(f, container), f))
    return out


def modes_cases(seed: int = 21) -> list:
    rng = np.random.default_rng(seed)
    return _group(_bases(seed), rng, random_modes, 2, "modes")


def filter_cases(seed: int = 22) -> list:
    rng = np.random.default_rng(seed)
    return _group(_bases(seed, golden_every=3), rng, filter_variant, 3, "filter")


def header_cases(seed: int = 23) -> list:
    rng = np.random.default_rng(seed)
    return _group(_bases(seed, golden_every=3), rng, header_variant, 3, "header")


def quant_down_cases(seed: int = 24) -> list:
    rng = np.random.default_rng(seed)
    bases = _bases(seed, golden_every=2) + pillow_bases(seed + 100, quality=(90, 101), sizes=BASE_SIZES[:12])
    return _group(bases, rng, quant_down_variant, 3, "qdown")


def quant_up_cases(seed: int = 25) -> list:
    rng = np.random.default_rng(seed)
    bases = pillow_bases(seed, kinds=("noisy", "drawing"), quality=(85, 96), sizes=BASE_SIZES[3:16])
    return _group(bases, rng, quant_up_variant, 4, "qup")


GROUPS = {"modes": modes_cases, "filter": filter_cases, "header": header_cases, "quant_down": quant_down_cases,
          "quant_up": quant_up_cases}


# ---- census ----------------------------------------------------------------------------------------------------------------
HEADER_FIELDS = ("lf_delta ref_lf[0]", "lf_delta mode_lf[0] with B_PRED", "segments relative", "segments without data update",
                 "segments without map update", "delta y1dc", "delta y2dc", "delta y2ac", "profile 3", "scale bits",
                 "colour space 1", "clamping 1", "quantiser index 0", "quantiser index 127", "segment prob 0",
                 "segment prob 255", "skip prob 0", "skip prob 255", "vp8x")
MODE_KEYS = tuple(f"{kind} {BMODE_NAMES[m]} {pos}" for kind, n in (("y16", 4), ("b4", 10), ("uv", 4)) for m in range(n)
                  for pos in POSITIONS)
LEVEL_KEYS = tuple(f"level {t} {lv}" for t in ("simple", "normal") for lv in FILTER_LEVELS) + tuple(
    f"sharpness {s}" for s in range(8))


def census(files) -> dict:
    """How many files carry each header field value, each (mode, position class) pair and each effective filter level."""
    c = dict.fromkeys(HEADER_FIELDS + MODE_KEYS + LEVEL_KEYS, 0)
    for item in files:
        data = item[1]
        f = parse(data)
        used = {(m["segment"], bool(m["is_i4"])) for m in f.mbs}
        hits = {"lf_delta ref_lf[0]": f.use_lf_delta and bool(f.ref_lf[0]),
                "lf_delta mode_lf[0] with B_PRED": f.use_lf_delta and bool(f.mode_lf[0]) and any(i4 for _, i4 in used),
                "segments relative": f.use_segment and f.update_data and not f.absolute,
                "segments without data update": f.use_segment and not f.update_data,
                "segments without map update": f.use_segment and not f.update_map,
                "delta y1dc": bool(f.dq[0]), "delta y2dc": bool(f.dq[1]), "delta y2ac": bool(f.dq[2]),
                "profile 3": f.profile == 3, "scale bits": bool(f.xscale or f.yscale), "colour space 1": f.color_space == 1,
                "clamping 1": f.clamping == 1,
                "quantiser index 0": any(quant_indices(f, s)[1] == 0 for s, _ in used),
                "quantiser index 127": any(quant_indices(f, s)[1] == 127 for s, _ in used),
                "segment prob 0": f.update_map and 0 in f.seg_probs, "segment prob 255": f.update_map and 255 in f.seg_probs,
                "skip prob 0": f.use_skip and f.skip_p == 0, "skip prob 255": f.use_skip and f.skip_p == 255,
                "vp8x": b"VP8X" in data[12:16]}
        keys = {k for k, v in hits.items() if v}
        if f.level:
            keys |= {f"level {'simple' if f.simple else 'normal'} {filter_level(f, s, i4)}" for s, i4 in used}
            keys.add(f"sharpness {f.sharpness}")
        for i, m in enumerate(f.mbs):
            for pos in position_classes(f, i % f.mb_w, i // f.mb_w):
                if m["is_i4"]:
                    keys |= {f"b4 {BMODE_NAMES[b]} {pos}" for b in m["bmodes"]}
                else:
                    keys.add(f"y16 {BMODE_NAMES[m['ymode']]} {pos}")
                keys.add(f"uv {BMODE_NAMES[m['uvmode']]} {pos}")
        for k in keys:
            if k in c:
                c[k] += 1
    return c


def encoded_fields(f: Frame) -> dict:
    """The values partition 0 and the frame tag carry, with what no flag writes left out: what parse() has to give back."""
    d = {k: v for k, v in vars(f).items() if k != "container"}
    if not f.use_segment:
        d.update(update_map=0, update_data=0)
    if not d["update_data"]:
        d.update(absolute=1, seg_quant=[None] * 4, seg_lf=[None] * 4)
    if not d["update_map"]:
        d["seg_probs"] = [None] * 3
    if not f.use_lf_delta:
        d["lf_update"] = 0
    if not d["lf_update"]:
        d.update(ref_lf=[None] * 4, mode_lf=[None] * 4)
    if not f.use_skip:
        d["skip_p"] = None
    d["mbs"] = [dict(m, segment=m["segment"] if d["update_map"] else 0, ymode=None if m["is_i4"] else m["ymode"],
                     bmodes=m["bmodes"] if m["is_i4"] else None) for m in f.mbs]
    return d


def big_frame_case(seed: int = 26, w: int = 2176, h: int = 1088) -> tuple:
    """(name, bytes): a frame wide and tall enough that a wavefront step of the GPU decoder holds more than 64 macroblocks,
    with random modes and the strongest normal filter on every segment."""
    rng = np.random.default_rng(seed)
    f = parse(W.pillow_file(W.content(rng, w, h, "drawing"), 80, 2))
    random_modes(f, rng)
    _segments_free(f, rng, 1)
    f.simple, f.level, f.sharpness = 0, 63, 0
    f.seg_lf = [63, 63, 41, 40]
    f.use_lf_delta, f.lf_update, f.ref_lf, f.mode_lf = 1, 1, [0, None, None, None], [-1, None, None, None]
    return f"big_modes_filtered_{w}x{h}", emit(f)
