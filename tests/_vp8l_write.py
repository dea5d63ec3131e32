"""A small VP8L (lossless WebP) writer for the tests of the lossless decoder (kobato-eyes_amd/csrc/ke_webpl_*.h, ke_webpl.hip):
it encodes pixels with features FORCED, because an encoder's own choices cannot be steered -- each predictor mode in a block of
its own, each transform alone and all four in several orders, transform block sizes 2..9 bits, the colour cache at given
sizes, an entropy image with many groups, simple and normal prefix codes, max_symbol, every short distance code, overlapping
and row-crossing copies, the longest length.  It does not try to compress.  Pillow is its check (test_webpl_cpu.py: every
written file decodes back to the pixels that went in), and ``CENSUS`` counts what was written -- by the writer, not by the
decoder under test.  Written from the published VP8L bitstream specification."""
from __future__ import annotations

import struct
from collections import Counter

import numpy as np

CENSUS: Counter = Counter()
PLANE = [0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
         0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
         0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
         0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
         0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
         0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70]
CL_ORDER = [17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
ALPHABET_NAMES = ("green", "red", "blue", "alpha", "distance")


def plane_distance(code: int, xsize: int) -> int:
    if code > 120:
        return code - 120
    e = PLANE[code - 1]
    return max((e >> 4) * xsize + 8 - (e & 15), 1)


class Bits:
    def __init__(self) -> None:
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value: int, nbits: int) -> None:
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def done(self) -> bytes:
        return bytes(self.out) + (bytes([self.acc & 255]) if self.n else b"")


# ---- prefix codes -------------------------------------------------------------------------------------------------------
def flat_lengths(used: list) -> dict:
    """A complete code over the used symbols with lengths k and k + 1."""
    n = len(used)
    if n == 1:
        return {used[0]: 1}
    k = n.bit_length() - 1
    short = (1 << (k + 1)) - n                                   # symbols of length k
    return {s: (k if i < short else k + 1) for i, s in enumerate(sorted(used))}


def canonical(lengths: dict) -> dict:
    """symbol -> (code bits reversed for the LSB-first stream, length); one used symbol: zero bits"""
    if len(lengths) == 1:
        return {next(iter(lengths)): (0, 0)}
    out, code, prev = {}, 0, 0
    for length, sym in sorted((l, s) for s, l in lengths.items()):
        code <<= length - prev
        prev = length
        out[sym] = (int(format(code, f"0{length}b")[::-1], 2), length)
        code += 1
    return out


def write_code(bw: Bits, used: list, alphabet: int, *, normal: bool = False, max_symbol: bool = False, name: str = "") -> dict:
    """Writes a code over the used symbols; returns symbol -> (bits, length)."""
    used = sorted(set(used)) or [0]
    if len(used) == 1:
        CENSUS[f"zero_bit_code_{name}"] += 1
    if len(used) <= 2 and max(used) < 256 and not normal:
        CENSUS[f"simple_code_{len(used)}_symbols"] += 1
        bw.put(1, 1)
        bw.put(len(used) - 1, 1)
        wide = used[0] > 1
        bw.put(int(wide), 1)
        bw.put(used[0], 8 if wide else 1)
        if len(used) == 2:
            bw.put(used[1], 8)
        return canonical({s: 1 for s in used})
    lengths = flat_lengths(used)
    bw.put(0, 1)
    seq = [lengths.get(s, 0) for s in range(alphabet)]
    if max_symbol:
        while seq and seq[-1] == 0:
            seq.pop()
    tokens, i, prev = [], 0, 8                                   # (code-length symbol, extra bits value, extra bits count)
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            run = min(run, 138)
            tokens.append((17, run - 3, 3) if run <= 10 else (18, run - 11, 7))
            CENSUS["repeat_code_17" if run <= 10 else "repeat_code_18"] += 1
        elif v != 0 and v == prev and run >= 3:
            run = min(run, 6)
            tokens.append((16, run - 3, 2))
            CENSUS["repeat_code_16"] += 1
        else:
            run = 1
            tokens.append((v, 0, 0))
        if v:
            prev = v
        i += run
    cl_code = canonical(flat_lengths(sorted({t[0] for t in tokens})))
    cl_len = flat_lengths(sorted({t[0] for t in tokens}))
    bw.put(19 - 4, 4)
    for s in CL_ORDER:
        bw.put(cl_len.get(s, 0), 3)
    if max_symbol:
        CENSUS["normal_code_max_symbol"] += 1
        bw.put(1, 1)
        count = len(tokens)
        nb = 2
        while count - 2 >= (1 << nb):
            nb += 2
        bw.put((nb - 2) // 2, 3)
        bw.put(count - 2, nb)
    else:
        CENSUS["normal_code"] += 1
        bw.put(0, 1)
    for s, extra, nextra in tokens:
        bw.put(*cl_code[s])
        bw.put(extra, nextra)
    return canonical(lengths)


def prefix_of(value: int):
    """length or distance code -> (prefix symbol, extra bits value, extra bits count)"""
    x = value - 1
    if x < 4:
        return x, 0, 0
    hb = x.bit_length() - 1
    extra = hb - 1
    return 2 * extra + 2 + ((x >> (hb - 1)) & 1), x & ((1 << extra) - 1), extra


# ---- one entropy-coded image --------------------------------------------------------------------------------------------
class Tokens:
    """The tokens of an image `xsize` wide, and the pixels they stand for, built together: lit() appends a pixel, copy() a
    back-reference into what is there already, fill() literal pixels (colour-cache hits where the cache holds them)."""

    def __init__(self, xsize: int, cache_bits: int = 0) -> None:
        self.xsize, self.cache_bits = xsize, cache_bits
        self.cache = [0] * (1 << cache_bits) if cache_bits else None
        self.pixels: list = []
        self.tokens: list = []                                   # (position, kind, ...)

    def _seen(self, argb: int) -> int:
        key = ((0x1e35a7bd * argb) & 0xFFFFFFFF) >> (32 - self.cache_bits)
        hit = self.cache[key] == argb
        self.cache[key] = argb
        return key if hit else -1

    def lit(self, argb: int) -> None:
        argb = int(argb)
        key = self._seen(argb) if self.cache is not None else -1
        if key >= 0:
            CENSUS["cache_hit"] += 1
            self.tokens.append((len(self.pixels), "cache", key))
        else:
            self.tokens.append((len(self.pixels), "lit", argb))
        self.pixels.append(argb)

    def fill(self, values) -> "Tokens":
        for v in values:
            self.lit(v)
        return self

    def copy(self, length: int, code: int) -> None:
        dist = plane_distance(code, self.xsize)
        pos = len(self.pixels)
        assert 1 <= dist <= pos and 1 <= length <= 4096
        CENSUS["copy"] += 1
        if code <= 120:
            CENSUS[f"distance_code_{code}"] += 1
        if dist < length:
            CENSUS["copy_overlapping_itself"] += 1
        if pos // self.xsize != (pos + length - 1) // self.xsize:
            CENSUS["copy_crossing_rows"] += 1
        if length == 4096:
            CENSUS["copy_length_4096"] += 1
        self.tokens.append((pos, "copy", length, code))
        for _ in range(length):
            v = self.pixels[len(self.pixels) - dist]
            if self.cache is not None:
                self._seen(v)
            self.pixels.append(v)


def write_image(bw: Bits, t: Tokens, ysize: int, *, main: bool, group_bits: int = 0, group_of=None, normal: bool = False,
                max_symbol: bool = False) -> None:
    """cache info, [entropy image], the groups' codes, the tokens"""
    assert len(t.pixels) == t.xsize * ysize
    bw.put(int(t.cache_bits > 0), 1)
    if t.cache_bits:
        bw.put(t.cache_bits, 4)
        CENSUS[f"colour_cache_{t.cache_bits}_bits"] += 1
    gw = 1
    if main:
        bw.put(int(group_bits > 0), 1)
    if group_bits:
        gw, gh = -(-t.xsize // (1 << group_bits)), -(-ysize // (1 << group_bits))
        gmap = [group_of(bx, by) for by in range(gh) for bx in range(gw)]
        CENSUS["entropy_image"] += 1
        CENSUS["entropy_image_groups_max"] = max(CENSUS["entropy_image_groups_max"], max(gmap) + 1)
        bw.put(group_bits - 2, 3)
        write_image(bw, Tokens(gw).fill(0xFF000000 | (g << 8) for g in gmap), gh, main=False)
    else:
        gmap = [0]

    def group_at(pos: int) -> int:
        return gmap[((pos // t.xsize) >> group_bits) * gw + ((pos % t.xsize) >> group_bits)] if group_bits else 0

    ngroups = max(gmap) + 1
    used = [[set() for _ in range(5)] for _ in range(ngroups)]
    for tok in t.tokens:
        u = used[group_at(tok[0])]
        if tok[1] == "lit":
            a = tok[2]
            u[0].add((a >> 8) & 255); u[1].add((a >> 16) & 255); u[2].add(a & 255); u[3].add(a >> 24)
        elif tok[1] == "cache":
            u[0].add(256 + 24 + tok[2])
        else:
            u[0].add(256 + prefix_of(tok[2])[0])
            u[4].add(prefix_of(tok[3])[0])
    codes = []
    for u in used:
        sizes = (256 + 24 + ((1 << t.cache_bits) if t.cache_bits else 0), 256, 256, 256, 40)
        codes.append([write_code(bw, sorted(u[j]), sizes[j], normal=normal, max_symbol=max_symbol, name=ALPHABET_NAMES[j]) for j in range(5)])
    for tok in t.tokens:
        c = codes[group_at(tok[0])]
        if tok[1] == "lit":
            a = tok[2]
            bw.put(*c[0][(a >> 8) & 255]); bw.put(*c[1][(a >> 16) & 255]); bw.put(*c[2][a & 255]); bw.put(*c[3][a >> 24])
        elif tok[1] == "cache":
            bw.put(*c[0][256 + 24 + tok[2]])
        else:
            s, extra, n = prefix_of(tok[2])
            bw.put(*c[0][256 + s]); bw.put(extra, n)
            s, extra, n = prefix_of(tok[3])
            bw.put(*c[4][s]); bw.put(extra, n)


# ---- the transforms, forwards ---------------------------------------------------------------------------------------------
def _avg2(a: int, b: int) -> int:
    return (((a ^ b) & 0xFEFEFEFE) >> 1) + (a & b)


def _channels(a: int):
    return [(a >> s) & 255 for s in (0, 8, 16, 24)]


def _join(ch) -> int:
    return sum((int(v) & 255) << s for v, s in zip(ch, (0, 8, 16, 24)))


def _clip(v: int) -> int:
    return 0 if v < 0 else 255 if v > 255 else v


def predict(mode: int, L: int, T: int, TL: int, TR: int) -> int:
    if mode == 0 or mode > 13:
        return 0xFF000000
    if mode <= 4:
        return (L, T, TR, TL)[mode - 1]
    if mode == 5:
        return _avg2(_avg2(L, TR), T)
    if mode in (6, 7, 8, 9):
        return _avg2(*{6: (L, TL), 7: (L, T), 8: (TL, T), 9: (T, TR)}[mode])
    if mode == 10:
        return _avg2(_avg2(L, TL), _avg2(T, TR))
    if mode == 11:
        dl = sum(abs(t - tl) for t, tl in zip(_channels(T), _channels(TL)))      # |p - L| with p = L + T - TL
        dt = sum(abs(l - tl) for l, tl in zip(_channels(L), _channels(TL)))
        return L if dl < dt else T
    if mode == 12:
        return _join(_clip(l + t - tl) for l, t, tl in zip(_channels(L), _channels(T), _channels(TL)))
    ave = _channels(_avg2(L, T))
    return _join(_clip(a + int((a - tl) / 2)) for a, tl in zip(ave, _channels(TL)))


def _sub(a: int, b: int) -> int:
    return _join((x - y) & 255 for x, y in zip(_channels(a), _channels(b)))


def forward_predictor(pix: list, w: int, h: int, bits: int, mode_of) -> tuple:
    bw_ = -(-w // (1 << bits))
    modes = [mode_of(bx, by) for by in range(-(-h // (1 << bits))) for bx in range(bw_)]
    out = list(pix)
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if y == 0:
                p = 0xFF000000 if x == 0 else pix[i - 1]
                CENSUS["predictor_top_row"] += 1
            elif x == 0:
                p = pix[i - w]
                CENSUS["predictor_left_column"] += 1
            else:
                m = modes[(y >> bits) * bw_ + (x >> bits)]
                CENSUS[f"predictor_mode_{m}"] += 1
                p = predict(m, pix[i - 1], pix[i - w], pix[i - w - 1], pix[i - w + 1])
            out[i] = _sub(pix[i], p)
    return out, [0xFF000000 | (m << 8) for m in modes], bw_


def _delta(m: int, c: int) -> int:
    m, c = (m ^ 128) - 128, (c ^ 128) - 128
    return (m * c) >> 5


def forward_cross(pix: list, w: int, h: int, bits: int, mult_of) -> tuple:
    bw_ = -(-w // (1 << bits))
    mults = [mult_of(bx, by) for by in range(-(-h // (1 << bits))) for bx in range(bw_)]     # (g2r, g2b, r2b)
    out = []
    for i, a in enumerate(pix):
        g2r, g2b, r2b = mults[((i // w) >> bits) * bw_ + ((i % w) >> bits)]
        b, g, r, al = _channels(a)
        out.append(_join(((b - _delta(g2b, g) - _delta(r2b, r)) & 255, g, (r - _delta(g2r, g)) & 255, al)))
    return out, [0xFF000000 | (r2b << 16) | (g2b << 8) | g2r for g2r, g2b, r2b in mults], bw_


def forward_green(pix: list) -> list:
    return [_join(((b - g) & 255, g, (r - g) & 255, a)) for b, g, r, a in map(_channels, pix)]


def forward_palette(pix: list, w: int, h: int, palette: list) -> tuple:
    n = len(palette)
    bits = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
    index = {c: i for i, c in reversed(list(enumerate(palette)))}
    per, pw = 8 >> bits, -(-w // (1 << bits))
    out = []
    for y in range(h):
        row = [0] * pw
        for x in range(w):
            row[x >> bits] |= index[pix[y * w + x]] << ((x & ((1 << bits) - 1)) * per)
        out += [0xFF000000 | (v << 8) for v in row]
    deltas = [palette[0]] + [_sub(palette[i], palette[i - 1]) for i in range(1, n)]
    CENSUS[f"palette_{8 >> bits}_bits_per_pixel"] += 1
    return out, deltas, pw


# ---- a whole file ---------------------------------------------------------------------------------------------------------
def write_file(w: int, h: int, pixels=None, *, transforms=(), tokens: Tokens = None, cache_bits: int = 0, group_bits: int = 0,
               group_of=None, normal: bool = False, max_symbol: bool = False, alpha: bool = False) -> bytes:
    """pixels: h*w ARGB values, run through ``transforms`` -- ("predictor", bits, mode_of), ("cross", bits, mult_of), ("green",),
    ("palette", colours) in stream order -- and written as literals (and cache hits); or ``tokens`` as built by the caller."""
    bw = Bits()
    bw.put(0x2F, 8); bw.put(w - 1, 14); bw.put(h - 1, 14); bw.put(int(alpha), 1); bw.put(0, 3)
    xs = w
    if tokens is None:
        pix = [int(v) for v in pixels]
        CENSUS["transforms_" + "_".join(t[0] for t in transforms) if transforms else "no_transform"] += 1
        for t in transforms:
            bw.put(1, 1)
            bw.put({"predictor": 0, "cross": 1, "green": 2, "palette": 3}[t[0]], 2)
            if t[0] in ("predictor", "cross"):
                pix, data, dw = (forward_predictor if t[0] == "predictor" else forward_cross)(pix, xs, h, t[1], t[2])
                CENSUS[f"{t[0]}_block_bits_{t[1]}"] += 1
                bw.put(t[1] - 2, 3)
                write_image(bw, Tokens(dw).fill(data), len(data) // dw, main=False)
            elif t[0] == "green":
                pix = forward_green(pix)
            else:
                colours = t[1] if t[1] is not None else sorted(set(pix))      # None: whatever the transforms before it left
                assert len(colours) <= 256
                pix, deltas, pw = forward_palette(pix, xs, h, colours)
                bw.put(len(colours) - 1, 8)
                write_image(bw, Tokens(len(deltas)).fill(deltas), 1, main=False)
                xs = pw
        tokens = Tokens(xs, cache_bits).fill(pix)
    bw.put(0, 1)
    write_image(bw, tokens, h, main=True, group_bits=group_bits, group_of=group_of, normal=normal, max_symbol=max_symbol)
    body = bw.done()
    body += b"\0" * (len(body) & 1)
    return b"RIFF" + struct.pack("<I", 12 + len(body)) + b"WEBPVP8L" + struct.pack("<I", len(body)) + body


def to_argb(a: np.ndarray) -> list:
    """h x w x 3 or 4 uint8 -> ARGB values"""
    a = a.astype(np.uint32)
    alpha = a[..., 3] if a.shape[-1] == 4 else np.uint32(255)
    return ((alpha << 24) | (a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2]).reshape(-1).tolist()


def to_rgba(pixels: list, w: int, h: int) -> np.ndarray:
    p = np.array(pixels, np.uint32).reshape(h, w)
    return np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255, p >> 24], -1).astype(np.uint8)


def written_cases(seed: int = 0) -> list:
    """[(name, file bytes, expected h x w x 4 RGBA pixels)]"""
    rng = np.random.default_rng(seed)
    out = []

    def image(w, h, kind="noisy", alpha=False):
        if kind == "noisy":
            a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        else:                                                    # few colours, smooth-ish
            yy, xx = np.mgrid[0:h, 0:w]
            a = np.stack([xx * 3 + yy, yy * 5, xx ^ yy, 255 - xx], -1).astype(np.uint8)
        if not alpha:
            a[..., 3] = 255
        return to_argb(a)

    def add(name, w, h, pix=None, **kw):
        data = write_file(w, h, pix, **kw)
        expected = pix if pix is not None else kw["tokens"].pixels
        out.append((name, data, to_rgba(expected, w, h)))

    # each predictor mode in blocks of its own, every block size
    for bits in range(2, 10):
        w, h = (37, 29) if bits < 6 else (70, 41)
        add(f"predictor_bits{bits}", w, h, image(w, h, "smooth" if bits % 2 else "noisy", alpha=bits == 3),
            transforms=[("predictor", bits, lambda bx, by, b=bits: (bx + 3 * by + b) % 14)])
    for mode in range(16):                                       # 14 and 15: no encoder writes them, the decoders predict black
        add(f"predictor_mode{mode}", 23, 19, image(23, 19, "noisy", alpha=True), transforms=[("predictor", 2, lambda bx, by, m=mode: m)])
    for bits in range(2, 10):
        add(f"cross_bits{bits}", 41, 33, image(41, 33), transforms=[("cross", bits, lambda bx, by: ((bx * 37 + 11) & 255, (by * 91 + 200) & 255, (bx + by) * 29 & 255))])
    add("green_alone", 31, 17, image(31, 17), transforms=[("green",)])
    for n in (1, 2, 3, 4, 5, 16, 17, 200, 256):
        pal = [int(v) for v in rng.integers(0, 1 << 32, n, dtype=np.uint64)]
        w, h = 45, 21
        pix = [pal[int(k)] for k in rng.integers(0, n, w * h)]
        add(f"palette_{n}", w, h, pix, transforms=[("palette", pal)])
    # all four, in several orders (after the palette the others work on the packed indices)
    pal = [int(v) for v in rng.integers(0, 1 << 32, 7, dtype=np.uint64)]
    orders = [("predictor", "cross", "green", "palette"), ("palette", "predictor", "cross", "green"), ("green", "predictor", "palette", "cross"),
              ("cross", "green", "predictor", "palette"), ("green", "palette", "cross", "predictor"), ("predictor", "palette", "green", "cross")]
    for k, order in enumerate(orders):
        w, h = 53 + k, 27 + k
        first = order[0] == "palette"
        pix = [pal[int(i)] for i in rng.integers(0, len(pal) if first else 2, w * h)]
        # (a palette further back has to hold what the transforms before it leave: neighbour-picking modes, one set of multipliers)
        spec = {"predictor": ("predictor", 2 + k % 3, (lambda bx, by: (5 * bx + by) % 14) if first else (lambda bx, by: 1 + (bx + by) % 4)),
                "cross": ("cross", 3, (lambda bx, by: (bx * 50 & 255, 77, by * 31 & 255)) if first else (lambda bx, by: (50, 77, 231))),
                "green": ("green",), "palette": ("palette", pal if first else None)}
        add(f"all_four_{k}", w, h, pix, transforms=[spec[n] for n in order], cache_bits=(0, 3, 0, 6, 0, 9)[k], group_bits=2 if k % 2 else 0,
            group_of=lambda bx, by: (bx + by) % 5)
    for order in (("green", "predictor"), ("predictor", "cross"), ("cross", "predictor", "green")):
        pix = image(40, 30, "smooth")
        spec = {"predictor": ("predictor", 3, lambda bx, by: (bx + by) % 14), "cross": ("cross", 2, lambda bx, by: (bx & 255, by & 255, 9)), "green": ("green",)}
        add("order_" + "_".join(order), 40, 30, pix, transforms=[spec[n] for n in order])
    # the colour cache
    for bits in (1, 5, 10, 11):
        pal = [int(v) | 0xFF000000 for v in rng.integers(0, 1 << 32, 40, dtype=np.uint64)]
        pix = [pal[int(i)] for i in rng.integers(0, len(pal), 50 * 30)]
        add(f"cache_{bits}", 50, 30, pix, cache_bits=bits)
    # an entropy image with many groups
    add("groups_many", 64, 64, image(64, 64), group_bits=2, group_of=lambda bx, by: by * 16 + bx)
    add("groups_sparse", 48, 40, image(48, 40, "smooth"), group_bits=3, group_of=lambda bx, by: (bx * 7 + by) % 11 * 3, cache_bits=4)
    add("groups_bits9", 600, 3, image(600, 3, "smooth"), group_bits=9, group_of=lambda bx, by: bx)
    # codes: flat images (zero-bit codes for every alphabet), two colours (simple codes), normal codes forced, max_symbol
    add("flat", 19, 11, [0x80123456] * (19 * 11), alpha=True)
    add("flat_normal_codes", 19, 11, [0xFF0000FE] * (19 * 11), normal=True)
    add("flat_1x1", 1, 1, [0xFFABCDEF])
    add("two_colours", 33, 9, [(0xFF000001, 0xFF010100)[int(i)] for i in rng.integers(0, 2, 33 * 9)])
    add("max_symbol", 30, 20, [0xFF000000 | int(v) for v in rng.integers(0, 9, 600)], max_symbol=True)
    add("max_symbol_cache", 30, 20, [0xFF000000 | int(v) << 9 for v in rng.integers(0, 30, 600)], max_symbol=True, cache_bits=7)
    # LZ77: every short distance code, overlapping copies, copies across rows, the longest length
    w = 24
    t = Tokens(w).fill(int(v) for v in rng.integers(0, 1 << 32, w * 9, dtype=np.uint64))
    for code in range(1, 121):
        t.copy(1 + code % 7, code)
        t.lit(int(rng.integers(0, 1 << 32)))
    while len(t.pixels) % w:
        t.lit(0xFF00FF00)
    add("distance_codes", w, len(t.pixels) // w, tokens=t)
    w = 5                                                        # narrow: codes whose x offset exceeds the width, distance clamped to 1
    t = Tokens(w).fill(int(v) for v in rng.integers(0, 1 << 32, w * 9, dtype=np.uint64))
    for code in range(1, 121):
        t.copy(2, code)
        t.lit(int(rng.integers(0, 1 << 32)))
    while len(t.pixels) % w:
        t.lit(1)
    add("distance_codes_narrow", w, len(t.pixels) // w, tokens=t)
    for bits in (0, 6):
        w = 100
        t = Tokens(w, bits).fill(int(v) for v in rng.integers(0, 1 << 32, 7, dtype=np.uint64))
        t.copy(4096, 121)                                        # distance 1: a run
        t.copy(4096, 120 + 3)                                    # period 3
        t.lit(5); t.lit(6)
        t.copy(300, 120 + 2)
        t.copy(977, 120 + 4000)                                  # far back, across many rows
        t.copy(1, 120 + len(t.pixels))                           # the first pixel
        for _ in range(200):
            t.copy(int(rng.integers(1, 40)), 120 + int(rng.integers(1, 500)))
            t.lit(int(rng.integers(0, 1 << 32)))
            t.lit(t.pixels[int(rng.integers(0, len(t.pixels)))])
        while len(t.pixels) % w:
            t.lit(0xFFFFFFFF)
        add(f"copies_cache{bits}", w, len(t.pixels) // w, tokens=t, alpha=True, group_bits=4 if bits else 0, group_of=lambda bx, by: (bx ^ by) & 3)
    return out


REQUIRED = ([f"predictor_mode_{m}" for m in range(14)] + ["predictor_top_row", "predictor_left_column"]
            + [f"predictor_block_bits_{b}" for b in range(2, 10)] + [f"cross_block_bits_{b}" for b in range(2, 10)]
            + ["transforms_predictor", "transforms_cross", "transforms_green", "transforms_palette", "no_transform"]
            + ["transforms_" + "_".join(o) for o in (("predictor", "cross", "green", "palette"), ("palette", "predictor", "cross", "green"),
                                                     ("green", "predictor", "palette", "cross"), ("cross", "green", "predictor", "palette"))]
            + [f"palette_{b}_bits_per_pixel" for b in (1, 2, 4, 8)] + [f"colour_cache_{b}_bits" for b in (1, 5, 10, 11)]
            + ["cache_hit", "entropy_image", "simple_code_1_symbols", "simple_code_2_symbols", "normal_code", "normal_code_max_symbol",
               "repeat_code_16", "repeat_code_17", "repeat_code_18"]
            + [f"distance_code_{c}" for c in range(1, 121)]
            + ["copy_overlapping_itself", "copy_crossing_rows", "copy_length_4096"] + [f"zero_bit_code_{n}" for n in ALPHABET_NAMES])
