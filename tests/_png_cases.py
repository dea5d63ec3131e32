"""PNG files for the decoder tests, made with the installed Pillow: what the GPU decoder takes (8-bit L / RGB / RGBA, every
compression level incl. stored blocks and optimised encoding, sizes from 1x1; palette, sub-byte, gray+alpha, Adam7 and 16-bit files)
and what it hands back (truncated, damaged, beyond its limits)."""
from __future__ import annotations

import io
import struct
import zlib

import numpy as np
from PIL import Image


def _save(arr, **kw) -> bytes:
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(arr)).save(b, "PNG", **kw)
    return b.getvalue()


def supported(full: bool = False):
    """Yields (name, file bytes, pixels as Pillow decodes them)."""
    rng = np.random.default_rng(3)
    sizes = [(1, 1), (2, 3), (7, 5), (64, 64), (101, 77), (300, 200), (512, 512)] + ([(1000, 31), (33, 1000), (1024, 768)] if full else [])
    for (w, h) in sizes:
        for kind in range(4):
            if kind == 0:
                a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            elif kind == 1:
                yy, xx = np.mgrid[0:h, 0:w]
                a = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) % 256, (xx * yy) % 256], -1).astype(np.uint8)
            elif kind == 2:
                base = rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 4), dtype=np.uint8)
                a = np.repeat(np.repeat(base, 16, 0), 16, 1)[:h, :w]
            else:
                a = np.full((h, w, 4), 200, np.uint8)
            for mode, arr in (("RGB", a[:, :, :3]), ("RGBA", a), ("L", a[:, :, 0])):
                for kw in ({}, {"compress_level": 0}, {"compress_level": 9}, {"optimize": True}) if full or kind == 2 else ({},):
                    data = _save(arr, **kw)
                    yield f"{w}x{h}_k{kind}_{mode}_{kw}", data, np.asarray(Image.open(io.BytesIO(data)))


def mapped(full: bool = False):
    """Yields (name, file bytes, luma as the reference's hashes see it: Image.open(...).convert("L")): palette files of every
    depth Pillow writes (2 / 4 / 16 / 256 colours -> 1 / 2 / 4 / 8 bits), with and without transparency, mode "1", and
    hand-packed 2- and 4-bit grayscale."""
    rng = np.random.default_rng(8)
    sizes = [(1, 1), (5, 3), (13, 9), (64, 64), (101, 77), (300, 200)] + ([(1000, 31), (33, 1000), (517, 389)] if full else [])
    for (w, h) in sizes:
        for ncol in (2, 4, 16, 256):
            pal = rng.integers(0, 256, ncol * 3, dtype=np.uint8)
            kinds = (0, 1) if full or (w, h) == (101, 77) else (0,)
            for kind in kinds:
                idx = rng.integers(0, ncol, (h, w), dtype=np.uint8) if kind == 0 else \
                    np.repeat(np.repeat(rng.integers(0, ncol, (h // 8 + 1, w // 8 + 1), dtype=np.uint8), 8, 0), 8, 1)[:h, :w]
                im = Image.fromarray(np.ascontiguousarray(idx), "P")
                im.putpalette(pal.tolist())
                for kw in ({}, {"transparency": 1}):
                    b = io.BytesIO()
                    im.save(b, "PNG", **kw)
                    data = b.getvalue()
                    yield f"P{ncol}_{w}x{h}_k{kind}_{kw}", data, np.asarray(Image.open(io.BytesIO(data)).convert("L"))
        b = io.BytesIO()
        Image.fromarray(rng.integers(0, 2, (h, w), dtype=np.uint8) * 255).convert("1").save(b, "PNG")
        data = b.getvalue()
        yield f"bilevel_{w}x{h}", data, np.asarray(Image.open(io.BytesIO(data)).convert("L"))
        la = np.stack([rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)], -1)
        if (w, h) == (101, 77):
            la[:, :, 0] = np.repeat(np.repeat(rng.integers(0, 256, (h // 8 + 1, w // 8 + 1), dtype=np.uint8), 8, 0), 8, 1)[:h, :w]
        for kw in ({}, {"compress_level": 9}) if full or (w, h) == (64, 64) else ({},):
            b = io.BytesIO()                                         # gray + alpha: the reference hashes convert("L") = the gray band
            Image.fromarray(la, "LA").save(b, "PNG", **kw)
            data = b.getvalue()
            yield f"LA_{w}x{h}_{kw}", data, np.asarray(Image.open(io.BytesIO(data)).convert("L"))
        for depth in (2, 4):                                         # grayscale below 8 bits: rows packed by hand
            per = 8 // depth
            vals = rng.integers(0, 1 << depth, (h, w), dtype=np.uint8)
            padded = np.zeros((h, (w + per - 1) // per * per), np.uint8)
            padded[:, :w] = vals
            packed = np.zeros((h, padded.shape[1] // per), np.uint8)
            for q in range(per):
                packed |= padded[:, q::per] << (8 - depth * (q + 1))
            rows = np.concatenate([rng.integers(0, 5, (h, 1), dtype=np.uint8), packed], 1)
            # the filter byte says how the row is stored; undo nothing here: store rows as filter 0 to keep the values as packed
            rows[:, 0] = 0
            data = _container(rows.tobytes(), w, h, 0, 6, 0, 1 << 30, depth=depth)
            yield f"gray{depth}_{w}x{h}", data, np.asarray(Image.open(io.BytesIO(data)).convert("L"))


def _container(raw: bytes, w: int, h: int, ctype: int, level: int, strategy: int, chunk: int, depth: int = 8, z: bytes = None,
               interlace: int = 0, plte: bytes = None) -> bytes:
    """A PNG around filtered scanlines given as they are, with control over what Pillow's writer never varies: the zlib
    strategy and the size of the IDAT chunks -- or around a ready zlib stream `z` (tests/_deflate_write.py)."""
    if z is None:
        co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
        z = co.compress(raw) + co.flush()

    def ch(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))

    out = [b"\x89PNG\r\n\x1a\n" + ch(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))]
    if plte is not None:
        out.append(ch(b"PLTE", plte))
    for o in range(0, len(z), chunk):
        out.append(ch(b"IDAT", z[o:o + chunk]))
    return b"".join(out) + ch(b"IEND", b"")


def handmade(full: bool = False):
    """Yields (name, file bytes, pixels as Pillow decodes them): streams Pillow's own writer does not produce -- code lengths
    up to 15 bits (a geometric byte histogram), Huffman-only / RLE / fixed-code / stored blocks, IDAT data cut into chunks
    of a few bytes, every filter type on random rows."""
    rng = np.random.default_rng(5)
    sizes = [(257, 129), (640, 480)] if full else [(257, 129)]
    for (w, h) in sizes:
        for ctype, ch_ in ((0, 1), (2, 3), (6, 4)):
            vals = np.minimum(rng.geometric(0.35, size=(h, w * ch_)) - 1, 255).astype(np.uint8)
            rows = np.concatenate([rng.integers(0, 5, (h, 1), dtype=np.uint8), vals], 1)
            for level, strategy, chunk in ((6, 0, 1 << 30), (9, zlib.Z_FILTERED, 4096), (1, zlib.Z_HUFFMAN_ONLY, 100), (6, zlib.Z_RLE, 7),
                                           (6, zlib.Z_FIXED, 1 << 30), (0, 0, 5000)):
                data = _container(rows.tobytes(), w, h, ctype, level, strategy, chunk)
                yield f"handmade_{w}x{h}_c{ctype}_l{level}_s{strategy}_k{chunk}", data, np.asarray(Image.open(io.BytesIO(data)))
    # copies of every short distance, overlapping their own output, in long dependent chains: row y repeats a random pattern
    # of (y % 24) + 1 bytes; then rows that repeat earlier rows at distances of a few hundred to a few thousand bytes
    for (w, h, ctype, ch_) in ((1200, 96, 0, 1), (401, 96, 2, 3), (16384, 3, 6, 4), (3, 4000, 2, 3)):
        rb = w * ch_
        body = np.empty((h, rb), np.uint8)
        for y in range(h):
            pat = rng.integers(0, 256, (y % 24) + 1, dtype=np.uint8)
            body[y] = np.resize(pat, rb)
        body[h // 2:] = body[: h - h // 2]
        rows = np.concatenate([np.zeros((h, 1), np.uint8), body], 1)
        for level in (6, 9):
            data = _container(rows.tobytes(), w, h, ctype, level, 0, 1 << 30)
            yield f"periodic_{w}x{h}_c{ctype}_l{level}", data, np.asarray(Image.open(io.BytesIO(data)))


_ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def _filtered(rows: np.ndarray, unit: int, types) -> bytes:
    """The forward PNG filters (specification, "Filter algorithms") on rows of packed bytes, one type per row."""
    h, rb = rows.shape
    out = bytearray()
    prev = np.zeros(rb, np.int32)
    for y in range(h):
        cur = rows[y].astype(np.int32)
        a = np.zeros(rb, np.int32)
        c = np.zeros(rb, np.int32)
        a[unit:] = cur[:rb - unit] if rb > unit else 0
        c[unit:] = prev[:rb - unit] if rb > unit else 0
        t = int(types[y])
        if t == 0:
            pred = 0
        elif t == 1:
            pred = a
        elif t == 2:
            pred = prev
        elif t == 3:
            pred = (a + prev) >> 1
        else:
            pa, pb, pc = np.abs(prev - c), np.abs(a - c), np.abs(a + prev - 2 * c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        out += bytes([t]) + ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def _adam7_stream(samples: np.ndarray, depth: int, rng, passes=_ADAM7) -> bytes:
    """samples: H x W x C (8-bit) or H x W x 1 values below 2**depth -> the seven passes' filtered rows, random filter types
    (passes=((0, 0, 1, 1),): the rows of a file without interlacing)."""
    h, w, ch = samples.shape
    out = b""
    for (x0, y0, dx, dy) in passes:
        sub = samples[y0::dy, x0::dx]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        if depth == 8:
            rows, unit = sub.reshape(sub.shape[0], -1), ch
        else:
            bits = ((sub[:, :, 0, None] >> np.arange(depth - 1, -1, -1)) & 1).reshape(sub.shape[0], -1).astype(np.uint8)
            rows, unit = np.packbits(bits, axis=1), 1
        out += _filtered(np.ascontiguousarray(rows), unit, rng.integers(0, 5, sub.shape[0]))
    return out


def _container2(raw: bytes, w: int, h: int, ctype: int, depth: int, interlace: int, plte: bytes = None, trns: bytes = None,
                level: int = 6, chunk: int = 1 << 30) -> bytes:
    def ch(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))

    z = zlib.compress(raw, level)
    out = b"\x89PNG\r\n\x1a\n" + ch(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))
    if plte is not None:
        out += ch(b"PLTE", plte)
    if trns is not None:
        out += ch(b"tRNS", trns)
    for o in range(0, len(z), chunk):
        out += ch(b"IDAT", z[o:o + chunk])
    return out + ch(b"IEND", b"")


def interlaced(full: bool = False):
    """Yields (name, file bytes, what the reference's hashes see): Adam7 files (no writer in Pillow -- built here, every filter
    type in every pass) of every kind the decoder takes: 8-bit L / RGB / RGBA / LA, palette and grayscale of 1 / 2 / 4 / 8 bits;
    sizes where some passes are empty (1x1 .. 4x4), where rows end inside a byte, and ordinary ones."""
    rng = np.random.default_rng(12)
    sizes = [(1, 1), (2, 1), (1, 2), (3, 2), (4, 4), (5, 5), (8, 8), (9, 17), (75, 53), (96, 80), (257, 129)] + ([(640, 333), (33, 1000), (1030, 40)] if full else [])
    for (w, h) in sizes:
        smooth = (w * h) > 5000
        for ctype, chans in ((0, 1), (2, 3), (6, 4), (4, 2)):
            if smooth:
                yy, xx = np.mgrid[0:h, 0:w]
                a = np.stack([(xx * 2 + yy) % 256, (yy * 3) % 256, (xx + yy // 2) % 256, (xx * yy // 7) % 256], -1).astype(np.uint8)[:, :, :chans]
                a = (a + rng.integers(0, 4, a.shape)).astype(np.uint8)
            else:
                a = rng.integers(0, 256, (h, w, chans), dtype=np.uint8)
            data = _container2(_adam7_stream(a, 8, rng), w, h, ctype, 8, 1, chunk=(1 << 30) if ctype != 2 else 37)
            with Image.open(io.BytesIO(data)) as im:
                ref = np.asarray(im.convert("L") if im.mode == "LA" else im)
            yield f"adam7_c{ctype}_{w}x{h}", data, ref
        for depth in (1, 2, 4, 8):
            vals = rng.integers(0, 1 << depth, (h, w, 1), dtype=np.uint8)
            for ctype in ((0, 3) if depth < 8 else (3,)):
                plte = rng.integers(0, 256, 3 * (1 << depth), dtype=np.uint8).tobytes() if ctype == 3 else None
                trns = bytes([0, 128]) if ctype == 3 and w % 2 else None
                data = _container2(_adam7_stream(vals, depth, rng), w, h, ctype, depth, 1, plte=plte, trns=trns)
                with Image.open(io.BytesIO(data)) as im:
                    ref = np.asarray(im.convert("L"))
                yield f"adam7_c{ctype}_d{depth}_{w}x{h}", data, ref


def wide(full: bool = False):
    """Yields (name, file bytes, what Pillow opens the file to -- for grayscale what convert("L") makes of its mode "I;16"):
    16-bit files of every colour type, with and without interlacing, every filter type (unit: 2 bytes per sample), samples
    with independent high and low bytes."""
    rng = np.random.default_rng(15)
    sizes = [(1, 1), (2, 3), (5, 4), (9, 17), (64, 48), (131, 67)] + ([(640, 333), (3, 900), (1030, 40)] if full else [])
    for (w, h) in sizes:
        for ctype, chans in ((0, 1), (2, 3), (4, 2), (6, 4)):
            a = rng.integers(0, 256, (h, w, 2 * chans), dtype=np.uint8)        # big-endian samples as bytes
            if ctype == 0:
                a[:, :, 0] = np.where(rng.random((h, w)) < 0.7, 0, a[:, :, 0])  # mostly below 256: convert("L") clips the rest
            if w * h > 3000:                                                    # something deflate finds matches in
                a[h // 4: h // 2] = a[h // 4]
            for lace in (0, 1):
                if lace:
                    raw = _adam7_stream(a, 8, rng)
                else:
                    raw = _filtered(np.ascontiguousarray(a.reshape(h, -1)), 2 * chans, rng.integers(0, 5, h))
                data = _container2(raw, w, h, ctype, 16, lace, chunk=(1 << 30) if ctype != 6 else 61)
                with Image.open(io.BytesIO(data)) as im:
                    ref = np.asarray(im.convert("L") if im.mode == "I;16" else im)
                yield f"wide_c{ctype}_{w}x{h}_i{lace}", data, ref


def animated(full: bool = False):
    """Yields (name, file bytes, what the reference's hashes see: frame 0 as Image.open shows it) for animated PNG files written
    by Pillow (the first frame is the IDAT image, or a separate default image is), and hand-edited ones: the file cut right
    behind frame 0's data, and what the decoder leaves to Pillow (expected = None: a first frame smaller than the image,
    a frame count of zero, a second acTL)."""
    rng = np.random.default_rng(21)
    sizes = [(7, 5), (64, 48), (101, 77)] + ([(300, 200)] if full else [])
    for (w, h) in sizes:
        frames = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(3)]
        frames[1][: h // 2] = frames[0][: h // 2]
        for mode in ("RGB", "RGBA", "L", "P"):
            ims = [Image.fromarray(f).convert("RGB").quantize(64) if mode == "P" else Image.fromarray(f).convert(mode) for f in frames]
            for default_image in (False, True):
                b = io.BytesIO()
                ims[0].save(b, "PNG", save_all=True, append_images=ims[1:], default_image=default_image, duration=80, loop=0)
                data = b.getvalue()
                with Image.open(io.BytesIO(data)) as im:
                    assert im.n_frames > 1
                    ref = np.asarray(im.convert("L") if im.mode in ("P", "1") else im)
                yield f"apng_{mode}_{w}x{h}_default{int(default_image)}", data, ref
                if mode == "RGB":
                    # nothing behind frame 0's data: Pillow stops reading at the next frame anyway
                    cut = data.index(b"fcTL", data.index(b"IDAT")) - 4
                    yield f"apng_cut_behind_frame0_{w}x{h}_default{int(default_image)}", data[:cut], ref
                    yield f"apng_cut_inside_next_fctl_{w}x{h}_default{int(default_image)}", data[:cut + 14], ref
    # left to Pillow
    b = io.BytesIO()
    ims = [Image.fromarray(rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)) for _ in range(2)]
    ims[0].save(b, "PNG", save_all=True, append_images=ims[1:])
    data = b.getvalue()

    def rechunk(at, body):
        n = struct.unpack(">I", data[at - 4:at])[0]
        t = data[at:at + 4]
        return data[:at + 4] + body + struct.pack(">I", zlib.crc32(t + body)) + data[at + 8 + n:]

    a = data.index(b"acTL")
    f = data.index(b"fcTL")
    fc = data[f + 4:f + 30]
    yield "apng_zero_frames", rechunk(a, struct.pack(">II", 0, 0)), None
    yield "apng_first_frame_smaller", rechunk(f, fc[:4] + struct.pack(">IIII", 30, 40, 0, 0) + fc[20:]), None
    yield "apng_first_frame_offset", rechunk(f, fc[:4] + struct.pack(">IIII", 49, 40, 1, 0) + fc[20:]), None
    yield "apng_sequence_from_1", rechunk(f, struct.pack(">I", 1) + fc[4:]), None
    actl = data[a - 4:a + 16]
    yield "apng_two_actl", data[:a - 4] + actl + actl + data[a + 16:], None


def refused():
    """Yields (name, file bytes, expected status): 1 = left to Pillow, 2 = damaged."""
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(a).convert("P").save(b, "PNG")
    pal = b.getvalue()
    cut = pal.index(b"PLTE") - 4
    n = struct.unpack(">I", pal[cut:cut + 4])[0]
    yield "palette_missing", pal[:cut] + pal[cut + 12 + n:], 2
    rng.integers(0, 65535, (20, 30))                                               # (keeps the stream of random numbers of earlier rounds)
    yield "16bit_beyond_the_row_limit", _container2(b"".join(b"\x00" + bytes(2 * 9000) for _ in range(2)), 9000, 2, 0, 16, 0), 1
    yield "16bit_palette", _container2(b"\x00" + bytes(8), 4, 1, 3, 16, 0, plte=bytes(6)), 1
    good = _save(rng.integers(0, 256, (40, 50, 3), dtype=np.uint8))
    yield "bad_adler", good[:-17] + bytes([good[-17] ^ 0x40]) + good[-16:], 2     # last byte of the zlib trailer (IDAT's CRC and the 12 bytes of IEND follow)
    yield "truncated", good[: len(good) // 2], 2
    yield "bit_flip_in_idat", good[:100] + bytes([good[100] ^ 1]) + good[101:], 2
    yield "not_a_png", b"GIF89a" + bytes(64), 2
    # IDAT, another chunk, IDAT: Pillow ends the stream at the first non-IDAT chunk ("image file is truncated"), the
    # reference's worker drops the file (src/core/fastsig.py:36-37)
    rows = np.concatenate([np.zeros((40, 1), np.uint8), rng.integers(0, 256, (40, 150), dtype=np.uint8)], 1).tobytes()
    whole = _container(rows, 50, 40, 2, 6, 0, 1 << 30)
    z_at = whole.index(b"IDAT") - 4
    zlen = struct.unpack(">I", whole[z_at:z_at + 4])[0]
    z = whole[z_at + 8:z_at + 8 + zlen]

    def ch(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))

    yield "idat_text_idat", whole[:z_at] + ch(b"IDAT", z[: zlen // 2]) + ch(b"tEXt", b"k\x00v") + ch(b"IDAT", z[zlen // 2:]) + ch(b"IEND", b""), 2


def random_handmade(n: int, seed: int = 0):
    """n random files of every colour type x bit depth x interlacing the decoder takes, every filter type, sizes up to
    120 x 90, IDAT data in chunks of random size: (name, file bytes, what the reference's hashes see)."""
    rng = np.random.default_rng(seed)
    kinds = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
    for k in range(n):
        w, h = int(rng.integers(1, 121)), int(rng.integers(1, 91))
        ctype, depth = kinds[int(rng.integers(0, len(kinds)))]
        lace = int(rng.integers(0, 2))
        chans = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
        if depth >= 8:
            a = rng.integers(0, 256, (h, w, chans * depth // 8), dtype=np.uint8)
            if rng.integers(0, 2):                                  # smooth content: matches, long filter chains
                a = (np.cumsum(rng.integers(0, 3, a.shape), 1) % 256).astype(np.uint8)
            if ctype == 0 and depth == 16:
                a[:, :, 0] = np.where(rng.random((h, w)) < 0.7, 0, a[:, :, 0])
            raw = _adam7_stream(a, 8, rng, _ADAM7 if lace else ((0, 0, 1, 1),))
        else:
            raw = _adam7_stream(rng.integers(0, 1 << depth, (h, w, 1), dtype=np.uint8), depth, rng, _ADAM7 if lace else ((0, 0, 1, 1),))
        plte = rng.integers(0, 256, 3 * int(rng.integers(1, (1 << depth) + 1)), dtype=np.uint8).tobytes() if ctype == 3 else None
        data = _container2(raw, w, h, ctype, depth, lace, plte=plte, level=int(rng.integers(0, 10)), chunk=int(rng.choice([7, 100, 8192, 1 << 30])))
        with Image.open(io.BytesIO(data)) as im:
            ref = np.asarray(im.convert("L") if im.mode in ("P", "1", "LA", "I;16") or (im.mode == "L" and depth < 8) else im)
        yield f"handmade{k}_c{ctype}_d{depth}_i{lace}_{w}x{h}", data, ref


def random_cases(n: int, seed: int = 0):
    """n random files of the kinds the decoder takes (sizes up to 200 x 150, every mode, compression level and texture):
    (name, file bytes, what the reference's hashes see)."""
    rng = np.random.default_rng(seed)
    for k in range(n):
        w, h = int(rng.integers(1, 201)), int(rng.integers(1, 151))
        mode = ("L", "RGB", "RGBA", "P", "1")[int(rng.integers(0, 5))]
        texture = int(rng.integers(0, 3))
        if texture == 0:
            a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        elif texture == 1:
            a = np.repeat(np.repeat(rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 4), dtype=np.uint8), 8, 0), 8, 1)[:h, :w]
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            a = np.stack([xx * 3 % 256, yy * 5 % 256, (xx + yy) % 256, (xx * yy) % 256], -1).astype(np.uint8)
        if mode == "P":
            im = Image.fromarray(np.ascontiguousarray(a[:, :, :3])).quantize(int(rng.integers(2, 257)))
        elif mode == "1":
            im = Image.fromarray(np.ascontiguousarray(a[:, :, 0])).convert("1")
        else:
            im = Image.fromarray(np.ascontiguousarray({"L": a[:, :, 0], "RGB": a[:, :, :3], "RGBA": a}[mode]))
        b = io.BytesIO()
        im.save(b, "PNG", compress_level=int(rng.integers(0, 10)), optimize=bool(rng.integers(0, 2)))
        data = b.getvalue()
        with Image.open(io.BytesIO(data)) as back:
            ref = np.asarray(back.convert("L") if back.mode in ("P", "1") else back)
        yield f"random{k}_{mode}_{w}x{h}", data, ref


# ---- hand-written deflate streams (tests/_deflate_write.py): what zlib's compressor never emits --------------------------------
# The judge of every case below is the installed zlib and Pillow, never the decoder: the valid and the random set assert here
# that zlib.decompress returns the intended bytes and that Pillow loads the file; the invalid set records what Pillow does.
import _deflate_write as D


def _row_geometry(n: int):
    """A one-row image whose filtered bytes are n bytes long: (width, colour type) or None.  With one row only the first byte
    is a filter type, so every other byte of the stream is free."""
    m = n - 1
    if 1 <= m <= 16384:
        return m, 0
    if m % 4 == 0 and m // 4 <= 16384:
        return m // 4, 6
    if m % 3 == 0 and m // 3 <= 16384:
        return m // 3, 2
    return None


def _pillow(data: bytes):
    """What Pillow's strict decode makes of the file: the pixels the reference's hashes see, or None where it refuses."""
    from PIL import ImageFile

    saved, ImageFile.LOAD_TRUNCATED_IMAGES = ImageFile.LOAD_TRUNCATED_IMAGES, False      # strict, as in the batch hasher's workers
    try:
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            return np.asarray(im.convert("L") if im.mode in ("P", "1", "LA", "I;16") else im)
    except Exception:
        return None
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = saved


def pixel_digest(a) -> str:
    """What two decodes of a file are compared by across processes: shape and bytes of the pixels, "-" for a refusal."""
    import hashlib

    return "-" if a is None else hashlib.sha1(repr(a.shape).encode() + a.tobytes()).hexdigest()


def _zlib_says(z: bytes):
    try:
        return zlib.decompress(z)
    except zlib.error:
        return None


def _deflate_file(blocks, chunk: int, raw: bytes = None, geometry=None, **wrap):
    """-> (file bytes, zlib stream, Stream): the blocks as a zlib stream in a PNG; raw: the filtered bytes the image is sized
    for and the Adler-32 is taken of (default: what the tokens mean); geometry: (w, h, ctype, depth, interlace, plte)."""
    s = D.Stream(blocks)
    raw = s.raw if raw is None else raw
    if geometry is None:
        w, ctype = _row_geometry(len(raw))
        geometry = (w, 1, ctype, 8, 0, None)
    w, h, ctype, depth, lace, plte = geometry
    z = D.zlib_wrap(s.bits, raw, **wrap)
    return _container(b"", w, h, ctype, 0, 0, chunk, depth=depth, z=z, interlace=lace, plte=plte), z, s


class _Tokens:
    """A token list that keeps count of the output: starts with a filter type and random literals."""

    def __init__(self, rng, head: int, top: int = 256) -> None:
        self.rng, self.top = rng, top
        self.t = [int(rng.integers(0, 5))]
        self.pos = 1
        self.lit(head - 1)

    def lit(self, n: int = 1):
        self.t += [int(v) for v in self.rng.integers(0, self.top, n)]
        self.pos += n
        return self

    def copy(self, length: int, dist: int, alt: bool = False):
        assert 3 <= length <= 258 and 1 <= dist <= self.pos, (length, dist, self.pos)
        self.t.append((length, dist, "284+31") if alt else (length, dist))
        self.pos += length
        return self


def _fit_head(body: int, least: int) -> int:
    head = least
    while _row_geometry(head + body) is None:
        head += 1
    return head


_COPY_LENGTHS = (3, 4, 15, 16, 17, 31, 32, 33, 257, 258)
_NEAR = tuple(range(1, 41)) + (255, 256, 257)
_RUNS = (2, 3, 5, 17, 63, 64, 65, 130, 200)                          # back-to-back copies of one distance


def _valid_streams():
    """Yields (name, blocks, extra census, keywords for the zlib wrapper)."""
    rng = np.random.default_rng(31)
    none = {}
    # ---- codes
    ll = [0] * 258
    for v in range(13):
        ll[v] = v + 1
    ll[13] = ll[14] = ll[256] = ll[257] = 15
    dd = [k + 1 for k in range(14)] + [15, 15]
    t = _Tokens(rng, 400, top=15)
    for ds in range(16):
        t.copy(3, D.DIST_BASE[ds]).lit(2)
    yield "codes_of_15_bits_in_both_alphabets", [D.dynamic(t.t, ll, dd, final=True)], none, none
    t = _Tokens(rng, 1, top=1)
    t.t = [0] * 40
    yield "two_literal_length_symbols_no_distance_code", [D.dynamic(t.t, D.flat_lengths([0, 256], 257), [0], final=True)], none, none
    t = _Tokens(rng, 1)
    t.t += list(range(256))
    t.pos += 256
    for k in range(29):                                              # every length symbol, every distance symbol
        t.copy(D.LEN_BASE[k], D.DIST_BASE[k] if D.DIST_BASE[k] <= t.pos else 1)
    for ds in range(30):
        t.lit(max(0, D.DIST_BASE[ds] + (1 << D.DIST_EXTRA[ds]) - t.pos))
        t.copy(3, D.DIST_BASE[ds]).copy(5, D.DIST_BASE[ds] + (1 << D.DIST_EXTRA[ds]) - 1).lit(1)
    t.lit(_fit_head(t.pos, 0))
    yield "all_286_literal_length_and_30_distance_symbols", [D.dynamic(t.t, D.flat_lengths(range(286), 286), D.flat_lengths(range(30), 30), final=True)], none, none
    t = _Tokens(rng, 30, top=3).copy(10, 1).lit(3).copy(4, 1).lit(2)
    yield "one_distance_symbol_of_1_bit", [D.auto_dynamic(t.t, final=True)], none, none
    t = _Tokens(rng, 30, top=3).copy(10, 1).lit(3).copy(4, 2).lit(2)
    yield "two_distance_symbols", [D.auto_dynamic(t.t, final=True)], none, none
    t = _Tokens(rng, 50)
    yield "empty_final_block_of_one_1_bit_code", [D.fixed(t.t), D.dynamic([], D.flat_lengths([256], 257), [0], final=True)], none, none
    yield "empty_blocks_of_every_type_in_front", [D.stored(b""), D.fixed([]), D.dynamic([], D.flat_lengths([256], 257), [0]), D.stored(b""),
                                                  D.fixed(t.t), D.stored(b"", final=True)], none, none
    t = _Tokens(rng, 90)
    blocks = []
    for k, v in enumerate(t.t):
        blocks.append((D.stored(bytes([v])), D.fixed([v]), D.auto_dynamic([v]))[k % 3])
    blocks[-1]["final"] = True
    yield "tiny_blocks_of_alternating_types", blocks, none, none
    # every length 3..258, 258 in both spellings
    t = _Tokens(rng, 300)
    for length in range(3, 259):
        t.copy(length, int(rng.integers(17, 300))).lit(int(rng.integers(0, 2)))
    t.copy(258, 40, alt=True).lit(1).copy(258, 3, alt=True)
    t.lit(_fit_head(t.pos, 0))
    yield "every_length_3_to_258", [D.auto_dynamic(t.t, final=True, rng=rng)], none, none
    # ---- stored blocks behind Huffman blocks that end at every bit, the stream ring inside stored blocks and headers
    t = _Tokens(rng, 1)
    blocks, tail = [D.fixed(t.t)], bytearray()
    for k in range(60):
        lits = [200] * (k // 2 % 8) + [int(v) for v in rng.integers(0, 144, int(rng.integers(1, 4)))]   # 9-bit codes shift the end by one bit each
        data = rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8).tobytes()
        blocks += [D.fixed(lits) if k % 2 else D.auto_dynamic(lits, rng=rng), D.stored(data)]
    blocks[-1]["final"] = True
    yield "stored_blocks_behind_every_bit_offset", blocks, none, none
    t = _Tokens(rng, 1)
    big = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
    yield "stored_block_of_65535_bytes", [D.fixed(t.t), D.stored(big), D.fixed([7], final=True)], none, none
    t = _Tokens(rng, 1)
    blocks = [D.fixed(t.t)]
    for k in range(6):
        blocks.append(D.stored(rng.integers(0, 256, 2000 + k, dtype=np.uint8).tobytes()))
        blocks.append(D.fixed([int(rng.integers(0, 256))]))
    blocks[-1]["final"] = True
    yield "stored_blocks_of_2000_bytes_between_literals", blocks, none, none
    t = _Tokens(rng, 41)
    blocks = [D.dynamic([v], D.flat_lengths(range(286), 286), D.flat_lengths(range(30), 30)) for v in t.t]
    blocks[-1]["final"] = True
    yield "40_dynamic_headers_in_a_row", blocks, {"dynamic_headers_in_a_row_40": 1}, none
    # the run-length encoding of a header: every repeat count of 16 / 17 / 18, a repeat that crosses into the distances
    t = _Tokens(rng, 8, top=4)
    for s, counts in ((16, range(3, 7)), (17, range(3, 11)), (18, range(11, 139))):
        for r in counts:
            ll = [0] * 286
            ll[0], ll[1], ll[2], ll[3] = 3, 3, 3, 3
            if s == 16:
                ll[4:4 + r + 1] = [0] * (r + 1)
                ops = [(3, None)] * 4 + [(0, None), (16, r)]
                at = 5 + r
            else:
                ops = [(3, None)] * 4 + [(s, r)]
                at = 4 + r
            ops += [(0, None)] * (256 - at)
            ll[256] = 1
            ops += [(1, None), (0, None)]                             # 256, then one distance length
            blocks = [D.dynamic(t.t, ll, [0], final=True, hlit=257, hdist=1, ops=ops)]
            yield f"header_repeat_{s}_times_{r}", blocks, none, none
    t = _Tokens(rng, 1)
    t.t = [0, 1, 1, 0, 1, 0, 0, (6, 1), (7, 2), 1, (6, 3), (7, 4), 0]
    ll = [2, 3] + [0] * 254 + [3, 0, 0, 0, 2, 2]                      # 0, 1, 256, 260, 261: the 2 of 261 repeats into the distances
    dd = [2, 2, 2, 2]
    yield "header_repeat_16_crosses_into_the_distances", [D.dynamic(t.t, ll, dd, final=True, ops=[(2, None), (3, None), (18, 138), (18, 116), (3, None),
                                                                   (0, None), (0, None), (0, None), (2, None), (16, 5)])], none, none
    t.t = [0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 1, (3, 9), 0]
    ll = [2, 2] + [0] * 254 + [2, 2] + [0] * 20
    dd = [0, 0, 0, 0, 0, 0, 1]
    yield "header_repeat_17_crosses_into_the_distances", [D.dynamic(t.t, ll, dd, final=True, hlit=278, ops=[(2, None), (2, None), (18, 138), (18, 116), (2, None), (2, None),
                                                                   (18, 16), (17, 10), (1, None)])], none, none
    ll = [2, 2] + [0] * 254 + [2, 2] + [0] * 28
    dd = [0] * 20 + [1]
    t.t = [0] + [1] * 1100 + [(3, 1025), 0]
    yield "header_repeat_18_crosses_into_the_distances", [D.dynamic(t.t, ll, dd, final=True, hlit=286, ops=[(2, None), (2, None), (18, 138), (18, 116), (2, None), (2, None),
                                                                   (18, 48), (1, None)])], none, none
    t = _Tokens(rng, 30, top=3).copy(4, 2).lit(2)
    lu, du = D.lengths_used(t.t)
    yield "header_with_trailing_zero_lengths_sent", [D.dynamic(t.t, D.flat_lengths(lu, 286), D.flat_lengths(du, 30), final=True, hlit=286, hdist=30, hclen=19)], none, none
    yield "header_with_trailing_zero_lengths_trimmed", [D.dynamic(t.t, D.flat_lengths(lu, 286), D.flat_lengths(du, 30), final=True)], none, none
    t = _Tokens(rng, 60, top=255)
    yield "header_with_5_code_length_code_lengths", [D.dynamic(t.t, [8] * 255 + [0, 8], [0], final=True)], none, none      # lengths 0 and 8 only
    # ---- copies
    for length in _COPY_LENGTHS:
        t = _Tokens(rng, 260)
        for d in _NEAR:
            t.copy(length, d).lit(int(rng.integers(1, 4)))
        yield f"copies_of_length_{length}_near", [D.auto_dynamic(t.t, final=True, rng=rng if length % 2 else None)], none, none
    body = sum(2 * n + 2 for n in _COPY_LENGTHS)
    t = _Tokens(rng, _fit_head(body, 32768))
    for length in _COPY_LENGTHS:
        t.copy(length, 32767).lit(1).copy(length, 32768).lit(1)
    yield "copies_from_32767_and_32768_back", [D.auto_dynamic(t.t, final=True)], none, none
    t = _Tokens(rng, 40)
    for d in range(1, 34):
        t.lit(d).copy(max(d + 1, 3), d).lit(1).copy(258, d).lit(2).copy(2 * d + 3, d).lit(1)
    yield "overlapping_copies_of_every_distance_to_33", [D.auto_dynamic(t.t, final=True, rng=rng)], none, none
    for d in list(range(1, 17)) + [17]:
        t = _Tokens(rng, 20)
        for n in _RUNS:
            t.lit(d + 1)
            for _ in range(n):
                t.copy(int(rng.integers(3, 12)) if n > 17 else int(rng.integers(3, 41)), d)
        yield f"runs_of_2_to_200_copies_of_distance_{d}", [D.fixed(t.t, final=True) if d % 3 == 0 else D.auto_dynamic(t.t, final=True, rng=rng)], none, none
    t = _Tokens(rng, 20)
    for d in range(1, 17):
        t.lit(d + 1)
        for _ in range(12):
            t.copy(int(rng.integers(3, 30)), d).lit(1)
        t.copy(int(rng.integers(3, 30)), d).copy(int(rng.integers(3, 30)), d).lit(1).copy(int(rng.integers(3, 30)), d).copy(5, d)
    yield "runs_broken_by_one_literal", [D.auto_dynamic(t.t, final=True)], none, none
    for d in range(1, 17):
        t = _Tokens(rng, d)
        for _ in range(int(rng.integers(1, 80))):
            t.copy(int(rng.integers(3, 41)), d)
        yield f"run_in_front_of_which_lie_only_{d}_bytes", [D.auto_dynamic(t.t, final=True, rng=rng)], none, none
    # copies that read what a copy 1..63 records earlier wrote (inside one group of 64)
    t = _Tokens(rng, 200)
    ncopy = 0

    def filler():
        nonlocal ncopy
        t.copy(3 + ncopy % 5, t.pos - int(rng.integers(1, 150)))     # reads the literal head only
        ncopy += 1

    for back in range(1, 64):
        while ncopy % 64 + back >= 64:
            filler()
        at = t.pos
        t.copy(24, t.pos - int(rng.integers(1, 150)))
        ncopy += 1
        for _ in range(back - 1):
            filler()
        off = int(rng.integers(0, 20))
        t.copy(int(rng.integers(3, 60)), t.pos - at - off)             # starts inside that copy's 24 bytes
        ncopy += 1
        if back % 4 == 0:
            t.lit(1)
    t.lit(_fit_head(t.pos, 0))
    yield "copies_that_read_a_copy_1_to_63_records_earlier", [D.auto_dynamic(t.t, final=True)], none, none
    # chains: every copy reads the one in front of it, far enough back not to be a run
    t = _Tokens(rng, 64)
    for k in range(150):
        t.copy(20, 20 + k % 7)
    yield "chain_of_150_dependent_copies", [D.auto_dynamic(t.t, final=True)], none, none
    # copies from and to every offset mod 4, literals on both sides (the dwords shared with literals)
    for far in (0, 1):
        t = _Tokens(rng, 64)
        for a in range(4):
            for length in (3, 4, 5, 6, 16, 17, 18, 19):
                t.lit((a - t.pos) % 4 + 4)
                t.copy(length, int(rng.integers(17, 60)) if far else int(rng.integers(1, 17)))
                t.lit(1)
        yield f"copies_at_every_offset_mod_4_{'far' if far else 'near'}", [D.fixed(t.t, final=True) if far else D.auto_dynamic(t.t, final=True)], none, none
    for head, d in ((1, 1), (3, 3), (4, 2), (6, 5), (8, 8)):
        t = _Tokens(rng, head)
        for k in range(2000):
            t.copy(3, d if head < 6 else int(rng.integers(1, head + 1)))
        yield f"only_copies_of_length_3_behind_{head}_literals", [D.auto_dynamic(t.t, final=True)], none, none
    # ---- images of many rows (these also go through the hashes): every byte is 0..4, so any of them may start a row
    for w, h, ctype, chans in ((40, 16, 0, 1), (32, 24, 2, 3), (64, 48, 6, 4)):
        total = h * (w * chans + 1)
        t = _Tokens(rng, 24, top=5)
        while t.pos < total - 300:
            d = int(rng.integers(1, 17)) if rng.integers(0, 2) else int(rng.integers(17, min(t.pos, 600) + 1))
            for _ in range(int(rng.integers(1, 5))):
                t.copy(int(rng.integers(3, 60)), min(d, t.pos))
            t.lit(int(rng.integers(0, 6)))
        t.lit(total - t.pos)
        yield f"rows_{w}x{h}_c{ctype}", [D.auto_dynamic(t.t, final=True, rng=rng)], {"image_of_16_rows_or_more": 1}, {"geometry": (w, h, ctype, 8, 0, None)}
    # ---- the zlib header: every window size and level; distances beyond the declared window
    for cinfo in range(8):
        for flevel in range(4):
            reach = min((256 << cinfo) + 1 + flevel, 32768)
            body = 3 + 1 + 258
            t = _Tokens(rng, _fit_head(body, reach))
            t.copy(3, reach).lit(1).copy(258, reach)
            extra = {f"cinfo_{cinfo}": 1, f"flevel_{flevel}": 1}
            if reach > (256 << cinfo):
                extra["distance_beyond_the_declared_window"] = 1
            yield f"zlib_header_cinfo_{cinfo}_flevel_{flevel}", [D.auto_dynamic(t.t, final=True) if flevel % 2 else D.fixed(t.t, final=True)], extra, {"cinfo": cinfo, "flevel": flevel}


def deflate_valid():
    """Yields (name, file bytes, pixels as Pillow decodes them, census): hand-written streams that zlib inflates to the
    intended bytes (asserted here, for every case), each with something zlib's compressor never emits or the GPU path treats
    specially.  One-row images: only the first byte is a filter type.  IDAT chunks of 1 byte, 7 bytes, and one chunk."""
    for k, (name, blocks, extra, wrap) in enumerate(_valid_streams()):
        n = sum(len(b["data"]) if b["type"] == 0 else len(b["tokens"]) for b in blocks)
        chunk = (1, 7, 1 << 30)[k % 3] if n < 3000 else (7, 1 << 30)[k % 2]
        data, z, s = _deflate_file(blocks, chunk, **wrap)
        assert _zlib_says(z) == s.raw, name
        ref = _pillow(data)
        assert ref is not None, name
        census = s.census + D.Counter(extra)
        census[f"idat_chunks_of_{chunk if chunk < 8 else 'everything'}"] += 1
        toks = [t for b in blocks for t in (list(b["data"]) if b["type"] == 0 else b["tokens"])]
        census += D.copy_census(toks)
        yield name, data, ref, census


#: what deflate_valid has to contain (tests/test_png_cpu.py holds its census against this list)
def deflate_valid_features():
    f = ["block_stored", "block_fixed", "block_dynamic", "stored_empty", "stored_full", "stored_some", "stored_final", "stored_not_final"]
    f += [f"stored_behind_bit_{k}" for k in range(8)]
    f += ["literal_length_longest_15", "distance_longest_15", "literal_length_symbols_1", "literal_length_symbols_2", "literal_length_symbols_286",
          "distance_symbols_0", "distance_symbols_1", "distance_symbols_2", "distance_symbols_30", "single_1_bit_distance_code",
          "single_1_bit_literal_length_code", "lengths_sent_one_by_one", "trailing_zero_lengths_sent", "trailing_zero_lengths_trimmed",
          "dynamic_headers_in_a_row_40", "blocks_of_one_symbol_of_alternating_types", "stored_2000_or_more", "chain_of_100_dependent_copies",
          "image_of_16_rows_or_more"]
    f += [f"hclen_{n}" for n in (5, 12, 14, 16, 18, 19)]
    f += [f"repeat_16_times_{r}" for r in range(3, 7)] + [f"repeat_17_times_{r}" for r in range(3, 11)] + [f"repeat_18_times_{r}" for r in range(11, 139)]
    f += [f"repeat_{s}_crosses_into_distances" for s in (16, 17, 18)]
    f += [f"length_{n}" for n in range(3, 259)] + ["length_258_as_285", "length_258_as_284_31"]
    f += [f"distance_code_{c}_{e}" for c in range(30) for e in ("low", "high")]
    f += [f"distance_{d}_length_{n}" for d in _NEAR + (32767, 32768) for n in _COPY_LENGTHS]
    f += [f"overlap_distance_{d}" for d in range(1, 34)]
    f += [f"run_of_{n}_copies_of_distance_{d}" for d in range(1, 18) for n in _RUNS]
    f += ["run_broken_by_one_literal",
          "run_head_reads_from_offset_0", "copies_over_64", "copies_over_128", "copy_ends_with_the_output", "only_length_3_copies_behind_a_short_head"]
    f += [f"source_written_{k}_copies_earlier" for k in range(1, 64)]
    f += [f"copy_from_mod4_{a}_to_mod4_{b}_between_literals" for a in range(4) for b in range(4)]
    f += [f"cinfo_{c}" for c in range(8)] + [f"flevel_{c}" for c in range(4)] + ["distance_beyond_the_declared_window"]
    f += ["idat_chunks_of_1", "idat_chunks_of_7", "idat_chunks_of_everything"]
    return f


def _invalid_streams():
    """Yields (name, blocks, intended filtered bytes, keywords for the zlib wrapper).  The base: 67 pixels in one row, a
    dynamic block with the first 24 bytes (a copy among them), then a fixed block with the rest.  Every case changes one field
    of it; what is wrong sits in the first block, so a reader meets it before the image is complete."""
    rng = np.random.default_rng(37)
    first = [0, 1, 1, 0, 1, 0, 1, 1, (5, 3), 0, 0, 1, (3, 7), 1, 0, 1, 0, 0]        # 24 bytes
    rest = [int(v) for v in rng.integers(0, 256, 44)]
    out = bytearray()
    D.expand(first + rest, out)
    raw = bytes(out)
    LL = [2, 2] + [0] * 254 + [2, 3, 0, 3]                             # 0, 1 | 256, 257 (length 3), 259 (length 5): complete
    DD = [0, 0, 1, 0, 0, 1]                                            # 2 (distance 3), 5 (distances 7, 8): complete
    ops = [(l, None) for l in LL + DD]
    tail = [D.fixed(rest, final=True)]

    def dyn(**kw):
        args = dict(tokens=first, ll=LL, dd=DD)
        args.update(kw)
        return [D.dynamic(**args)] + tail

    yield "base_unchanged", dyn(), raw, {}
    # over-subscribed and incomplete sets
    yield "literal_length_code_over_subscribed", dyn(ll=[2, 2] + [0] * 254 + [2, 2, 0, 3]), raw, {}
    yield "distance_code_over_subscribed", dyn(dd=[0, 1, 1, 0, 0, 1]), raw, {}
    yield "literal_length_code_of_two_codes_incomplete", dyn(ll=[2] + [0] * 255 + [2], tokens=[0] * 24), bytes(24) + raw[24:], {}
    yield "literal_length_code_of_three_codes_incomplete", dyn(ll=[2, 2] + [0] * 254 + [2], tokens=[0, 1, 1, 0] * 6), bytes([0, 1, 1, 0] * 6) + raw[24:], {}
    yield "literal_length_code_incomplete_by_one_longer_code", dyn(ll=[2, 2] + [0] * 254 + [2, 3, 0, 4]), raw, {}
    yield "distance_code_of_two_codes_incomplete", dyn(dd=[0, 0, 2, 0, 0, 1]), raw, {}
    yield "distance_code_of_two_codes_incomplete_unused", dyn(dd=[0, 0, 2, 0, 0, 1], tokens=[0, 1, 1, 0] * 6), bytes([0, 1, 1, 0] * 6) + raw[24:], {}
    for n in range(2, 16):
        # one code of n bits: for 256 alone (an empty block in front), for one distance (used and unused)
        yield f"literal_length_code_of_one_{n}_bit_code", [D.dynamic([], [0] * 256 + [n], [0])] + [D.fixed(first + rest, final=True)], raw, {}
        yield f"distance_code_of_one_{n}_bit_code", dyn(dd=[0, 0, n], tokens=[0, 1, 1, 0, 1, 0, 1, 1, (5, 3), 0, 0, 1, (3, 3), 1, 0, 1, 0, 0]), \
            raw[:16] + raw[13:16] + raw[19:], {}
        yield f"distance_code_of_one_{n}_bit_code_unused", dyn(dd=[0, 0, n], tokens=[0, 1, 1, 0] * 6), bytes([0, 1, 1, 0] * 6) + raw[24:], {}
    yield "literal_length_code_of_one_1_bit_code_for_a_literal", [D.dynamic([], [1] + [0] * 256, [0], eob=False)] + [D.fixed(first + rest, final=True)], raw, {}
    # the code length code
    used = sorted({s for s, _ in ops})                                 # 0, 1, 2, 3
    for n in range(1, 8):
        cl = [0] * 19
        cl[0] = n
        yield f"code_length_code_of_one_{n}_bit_code", dyn(cl=cl, ops=[(0, None)] * len(ops)), raw, {}
    cl = D.flat_lengths(used, 19)
    yield "code_length_code_of_three_codes_incomplete", dyn(cl=[2, 2, 2, 0] + [0] * 15, ops=[(min(s, 2), None) for s, _ in ops]), raw, {}
    cl[3] = 3
    yield "code_length_code_incomplete_by_one_longer_code", dyn(cl=cl), raw, {}
    cl = D.flat_lengths(used, 19)
    cl[3] = 1
    yield "code_length_code_over_subscribed", dyn(cl=cl), raw, {}
    # the run-length encoding of the lengths
    cl5 = D.flat_lengths([0, 1, 2, 3, 16, 17, 18], 19)
    yield "repeat_16_first", dyn(cl=cl5, ops=[(16, 3)] + ops[3:]), raw, {}
    yield "repeat_16_first_base", dyn(cl=cl5), raw, {}
    # ... where the three lengths it stands for are zeros: a reader that lets "the length in front" default to 0 takes it
    high = [3, 4, 4, 3, 4, 3, 3, 4] * 3
    ll34 = [0, 0, 0, 2, 2] + [0] * 251 + [1]
    cl34 = D.flat_lengths([0, 1, 2, 16, 17], 19)
    for s in (16, 17):
        yield f"repeat_{s}_first_for_three_zero_lengths", [D.dynamic(high, ll34, [0], cl=cl34, ops=[(s, 3), (2, None), (2, None)] + [(0, None)] * 251 + [(1, None), (0, None)])] + tail, \
            bytes(high) + raw[24:], {}
    short = D.rle_ops(LL + DD)
    yield "repeats_base", dyn(cl=cl5, ops=short), raw, {}
    for s in (16, 17, 18):
        # the last lengths replaced by a repeat that runs one past HLIT + HDIST
        r = {16: 3, 17: 3, 18: 11}[s]
        yield f"repeat_{s}_runs_past_the_lengths", dyn(cl=cl5, ops=ops[:len(ops) - r + 1] + [(s, r)]), raw, {}
    yield "end_of_block_code_missing", [D.dynamic(list(raw), D.flat_lengths(range(256), 257), DD, final=True, eob=False)], raw, {}
    yield "end_of_block_code_missing_base", [D.dynamic(list(raw), D.flat_lengths(range(257), 257), DD, final=True)], raw, {}
    # fixed blocks: the symbols that have codes and no meaning
    for s in (286, 287):
        yield f"fixed_block_symbol_{s}", [D.fixed(first + [("sym", s)]), D.fixed(rest, final=True)], raw, {}
    for s in (30, 31):
        yield f"fixed_block_distance_{s}", [D.fixed(first[:12] + [("raw", 257, 0, s, 0)] + first[13:])] + tail, raw, {}
    for hlit in (287, 288):
        yield f"hlit_{hlit}", dyn(hlit=hlit), raw, {}
        yield f"hlit_{hlit}_with_a_code", dyn(ll=LL + [0] * (hlit - 1 - len(LL)) + [3], hlit=hlit), raw, {}
    for hdist in (31, 32):
        yield f"hdist_{hdist}", dyn(hdist=hdist), raw, {}
        yield f"hdist_{hdist}_with_a_code", dyn(dd=[0, 0, 1] + [0] * (hdist - 4) + [1], hdist=hdist, tokens=[0, 1, 1, 0, 1, 0, 1, 1, (5, 3)] + [0, 1] * 5 + [0]),\
            raw[:13] + bytes([0, 1] * 5 + [0]) + raw[24:], {}
    yield "hlit_286_hdist_30", dyn(hlit=286, hdist=30), raw, {}
    # stored blocks, block type 3
    for bit in (0, 7, 8, 15):
        yield f"stored_nlen_bit_{bit}_wrong", [D.stored(raw[:24], nlen=(24 ^ 0xFFFF) ^ (1 << bit))] + tail, raw, {}
    yield "stored_len_one_more_than_nlen_says", [D.stored(raw[:24], len_=25)] + tail, raw, {}
    yield "block_type_3", dyn(btype=3), raw, {}
    yield "block_type_3_final_and_empty_in_front", [D.dynamic([], D.flat_lengths([256], 257), [0], btype=3)] + [D.fixed(first + rest, final=True)], raw, {}
    # the zlib header
    good = [D.fixed(first + rest, final=True)]
    yield "zlib_fdict", good, raw, {"fdict": 1}
    yield "zlib_cinfo_8", good, raw, {"cinfo": 8}
    yield "zlib_cinfo_15", good, raw, {"cinfo": 15}
    yield "zlib_method_7", good, raw, {"cm": 7}
    yield "zlib_method_9", good, raw, {"cm": 9}
    yield "zlib_fcheck_one_more", good, raw, {"fcheck": (31 - 0x7880 % 31) % 31 + 1}
    yield "zlib_fcheck_zero", good, raw, {"fcheck": 0}
    yield "adler_wrong_in_the_last_byte", good, raw, {"adler": zlib.adler32(raw) ^ 1}
    yield "adler_wrong_in_the_first_byte", good, raw, {"adler": zlib.adler32(raw) ^ (1 << 31)}
    # distances and lengths against the output
    yield "distance_one_beyond_the_output_at_the_start", [D.fixed([0, 1, 1, (3, 4)] + first[3:])] + tail, raw, {}
    yield "distance_one_beyond_the_output_later", [D.fixed(first + rest[:20] + [(3, 45)] + rest[23:], final=True)], raw, {}
    yield "distance_equal_to_the_output_so_far", [D.fixed(first + rest[:20] + [(3, 44)] + rest[20:41], final=True)], raw[:44] + raw[:3] + raw[44:65], {}
    yield "distance_one_beyond_the_output_in_the_first_token", [D.fixed([(3, 1)] + first[3:])] + tail, raw, {}
    long = raw + raw[-1:]
    yield "literal_one_byte_past_the_image", [D.fixed(first + rest + [rest[-1]], final=True)], raw, {"adler": zlib.adler32(long)}
    yield "copy_one_byte_past_the_image", [D.fixed(first + rest[:-2] + [(3, 1)], final=True)], raw[:-2] + raw[-3:-2] * 2, {"adler": zlib.adler32(raw[:-2] + raw[-3:-2] * 3)}
    yield "stored_block_one_byte_past_the_image", [D.fixed(first), D.stored(raw[24:] + b"\x07", final=True)], raw, {"adler": zlib.adler32(raw + b"\x07")}
    yield "output_one_byte_short", [D.fixed(first + rest[:-1], final=True)], raw, {"adler": zlib.adler32(raw[:-1])}
    yield "block_behind_the_image", [D.fixed(first + rest), D.fixed([], final=True)], raw, {}
    yield "damaged_block_behind_the_image", [D.fixed(first + rest), D.dynamic([], [0] * 256 + [2], [0], btype=3, final=True)], raw, {}
    for cut in (1, 2, 4, 5, 6, 12):
        yield f"stream_ends_{cut}_bytes_short", good, raw, {"cut": cut}
    yield "stream_without_a_final_block", [D.fixed(first + rest)], raw, {}
    for tail_bytes in (b"\x00", b"\xff" * 9, raw[:30]):
        yield f"{len(tail_bytes)}_bytes_behind_the_trailer", good, raw, {"tail": tail_bytes}


def deflate_invalid():
    """Yields (name, file bytes, the pixels Pillow decodes or None where Pillow refuses the file, what zlib.decompress says
    of the stream: True / False): one stream per rule of RFC 1950 / 1951 a decoder has to hold, each differing from a valid
    stream in one field (the unchanged bases are among them), in IDAT chunks of 1 byte, 7 bytes, and one chunk."""
    for name, blocks, raw, wrap in _invalid_streams():
        for chunk, tag in ((1, "idat_1"), (7, "idat_7"), (1 << 30, "idat_whole")):     # (where Pillow stops reading depends on it)
            data, z, _ = _deflate_file(blocks, chunk, raw=raw, **wrap)
            yield f"{name}_{tag}", data, _pillow(data), _zlib_says(z) is not None


def _random_tokens(raw: bytes, rng) -> list:
    """A random parse of the bytes into literals and matches that are really there: candidates are the last places of the
    next three bytes, the distance of the copy in front (back-to-back copies of one distance) and short distances."""
    a = np.frombuffer(raw, np.uint8)
    n, p, toks, seen, last = len(raw), 0, [], {}, 0
    eager = float(rng.choice([0.3, 0.8, 1.0]))
    while p < n:
        tok = None
        if p + 3 <= n and p > 0 and rng.random() < eager:
            key = raw[p:p + 3]
            cands = [d for d in (last, seen.get(key, p + 1) and p - seen.get(key, -1), int(rng.integers(1, 17))) if 0 < d <= min(p, 32768)]
            rng.shuffle(cands)
            for d in cands:
                m = min(258, n - p)
                ne = np.flatnonzero(a[p:p + m] != a[p - d:p - d + m])
                top = int(ne[0]) if len(ne) else m
                if top >= 3:
                    length = top if rng.integers(0, 3) else int(rng.integers(3, top + 1))
                    tok, last = (length, d), d
                    break
        if tok is None:
            if p + 3 <= n:
                seen[raw[p:p + 3]] = p
            toks.append(raw[p])
            p += 1
        else:
            for q in range(p, min(p + tok[0], n - 2), 7):
                seen[raw[q:q + 3]] = q
            toks.append(tok)
            p += tok[0]
    return toks


def _random_blocks(raw: bytes, rng) -> list:
    toks, blocks, at, pos = _random_tokens(raw, rng), [], 0, 0
    while at < len(toks) or not blocks:
        kind = int(rng.integers(0, 6))
        if kind == 0:                                                # a stored block: bytes as they are
            n = int(rng.integers(0, 400))
            take = []
            while at < len(toks) and isinstance(toks[at], int) and len(take) < n:
                take.append(toks[at])
                at += 1
            blocks.append(D.stored(bytes(take)))
            continue
        n = int(rng.choice([1, 5, 60, 700, 1 << 20]))
        part = toks[at:at + n]
        at += n
        blocks.append(D.fixed(part) if kind == 1 else D.auto_dynamic(part, rng=rng, limit=int(rng.choice([7, 9, 12, 15]))))
    blocks[-1]["final"] = True
    return blocks


def _random_image(rng, big: bool):
    """-> (filtered bytes, geometry) of a random image of the kinds random_handmade makes, with content deflate finds
    matches in."""
    kinds = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
    w, h = (int(rng.integers(1, 301)), int(rng.integers(1, 201))) if big else (int(rng.integers(1, 49)), int(rng.integers(1, 33)))
    ctype, depth = kinds[int(rng.integers(0, len(kinds)))]
    lace = int(rng.integers(0, 2))
    chans = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    texture = int(rng.integers(0, 4))
    shape = (h, w, chans * depth // 8) if depth >= 8 else (h, w, 1)
    top = 256 if depth >= 8 else 1 << depth
    if texture == 0:
        a = rng.integers(0, top, shape, dtype=np.uint8)
    elif texture == 1:
        a = (np.cumsum(rng.integers(0, 3, shape), 1) % top).astype(np.uint8)
    elif texture == 2:
        a = np.repeat(np.repeat(rng.integers(0, top, (h // 8 + 1, w // 8 + 1, shape[2]), dtype=np.uint8), 8, 0), 8, 1)[:h, :w]
    else:
        a = np.tile(rng.integers(0, top, (1, int(rng.integers(1, 6)), shape[2]), dtype=np.uint8), (h, w, 1))[:, :w]
    if ctype == 0 and depth == 16:
        a[:, :, 0] = np.where(rng.random((h, w)) < 0.7, 0, a[:, :, 0])
    raw = _adam7_stream(np.ascontiguousarray(a), 8 if depth >= 8 else depth, rng, _ADAM7 if lace else ((0, 0, 1, 1),))
    plte = rng.integers(0, 256, 3 * (1 << depth), dtype=np.uint8).tobytes() if ctype == 3 else None
    return raw, (w, h, ctype, depth, lace, plte)


def deflate_random(n: int, seed: int = 0):
    """n random block lists around the filtered rows of random images (every colour type x bit depth x interlacing of
    random_handmade, sizes up to 300 x 200, one in sixteen large): random complete codes from random length-limited trees,
    random header encodings, random parses with a bias to short distances and back-to-back copies, stored / fixed / dynamic
    blocks in any order.  Yields (name, file bytes, what the reference's hashes see); zlib and Pillow are asserted on every one."""
    rng = np.random.default_rng(seed)
    for k in range(n):
        raw, geometry = _random_image(rng, k % 16 == 7)
        blocks = _random_blocks(raw, rng)
        data, z, s = _deflate_file(blocks, int(rng.choice([1, 7, 1 << 30])) if len(raw) < 4000 else int(rng.choice([7, 1 << 30])), raw=raw, geometry=geometry)
        assert s.raw == raw and _zlib_says(z) == raw, k
        ref = _pillow(data)
        assert ref is not None, k
        w, h, ctype, depth, lace, _ = geometry
        yield f"deflate_random{k}_c{ctype}_d{depth}_i{lace}_{w}x{h}", data, ref


def deflate_header_fuzz(bases: int, per_base: int, seed: int = 0):
    """Single fields of a dynamic block's header rewritten, everything behind it bit for bit as it was: one code length of the
    code length code, one sent length, one repeat count, HLIT / HDIST / HCLEN, each by +-1.  The Adler-32 and the chunk
    checksum are set right for whatever zlib inflates the stream to, so that only the deflate layer can object.
    bases x per_base files, each a real rewrite.  Yields (name, file bytes, Pillow's pixels or None, whether zlib inflates the
    whole stream to exactly the image's bytes -- Pillow stops reading at the last row and never sees what lies behind it)."""
    rng = np.random.default_rng(seed)
    for b in range(bases):
        raw, geometry = _random_image(rng, False)
        toks = _random_tokens(raw, rng)
        blk = D.auto_dynamic(toks, final=True, rng=rng, limit=int(rng.choice([7, 11, 15])))
        if "ops" not in blk or all(s < 16 for s, _ in blk["ops"]):
            blk = D.dynamic(toks, blk["ll"], blk["dd"], final=True, ops=D.rle_ops((blk["ll"] + [0] * 288)[:blk["hlit"]] + (blk["dd"] + [0] * 32)[:blk["hdist"]]),
                            hlit=blk["hlit"], hdist=blk["hdist"])
        k = 0
        while k < per_base:                                           # a draw that changes nothing (a field at its limit) is drawn again
            m = dict(blk, cl=list(blk["cl"]), ops=list(blk["ops"]))
            field = int(rng.integers(0, 6))
            step = int(rng.choice([-1, 1]))
            if field == 0:
                s = D.CL_ORDER[int(rng.integers(0, m["hclen"]))]
                m["cl"][s] = min(7, max(0, m["cl"][s] + step))
            elif field == 1:
                m["hlit"] = min(288, max(257, m["hlit"] + step))
            elif field == 2:
                m["hdist"] = min(32, max(1, m["hdist"] + step))
            elif field == 3:
                m["hclen"] = min(19, max(4, m["hclen"] + step))
            else:
                want = field == 4
                idx = [i for i, (s, _) in enumerate(m["ops"]) if (s < 16) == want]
                if not idx:
                    continue
                i = idx[int(rng.integers(0, len(idx)))]
                s, r = m["ops"][i]
                if s < 16:
                    s = s + step
                    if not 0 <= s < 16 or not m["cl"][s]:
                        continue
                else:
                    lo, hi = {16: (3, 6), 17: (3, 10), 18: (11, 138)}[s]
                    r = min(hi, max(lo, r + step))
                m["ops"][i] = (s, r)
            if m == blk:
                continue
            k += 1
            bits = D.Stream([m]).bits
            try:
                got = zlib.decompressobj(-15).decompress(bits)
            except zlib.error:
                got = None
            z = D.zlib_wrap(bits, got if got is not None else raw)
            w, h, ctype, depth, lace, plte = geometry
            data = _container(b"", w, h, ctype, 0, 0, 1 << 30, depth=depth, z=z, interlace=lace, plte=plte)
            yield f"header_fuzz_{b}_{k}_field{field}{step:+d}", data, _pillow(data), got is not None and len(got) == len(raw)
