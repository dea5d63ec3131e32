"""Compressed TIFF files for the decoder tests (ke_tiffc_*): what Pillow / libtiff write with LZW and PackBits, with and
without the horizontal predictor; hand-made directories (tests/_tiff_cases.tiff) around strips from the tests' own writers
(tests/_lzw_write.py) for what libtiff never writes; the files that must be refused, each with its status; and damage."""
from __future__ import annotations

import io
import struct

import numpy as np
from PIL import Image, ImageDraw, ImageFile

import _lzw_write as Z
import _tiff_cases as T

OK, UNSUPPORTED, CORRUPT = 0, 1, 2
LZW, PACKBITS = 5, 32773


def pillow_pixels(data: bytes):
    """What the reference's hashes see of the file, strictly (a truncated file raises): None where Pillow raises."""
    was = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = False
    try:
        return T._pillow(data)
    except Exception:
        return None
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = was


def content(rng, w: int, h: int, kind: str) -> np.ndarray:
    """h x w x 4: noise, a smooth gradient with a little texture, or a flat drawing."""
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if kind == "smooth":
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1), 255 - (x * 200) // max(w - 1, 1)], -1)
        return (a + rng.integers(0, 3, (h, w, 4))).clip(0, 255).astype(np.uint8)
    im = Image.new("RGBA", (w, h), (250, 250, 245, 255))
    d = ImageDraw.Draw(im)
    for _ in range(6):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        d.rectangle([x0, y0, x0 + int(rng.integers(1, w + 1)), y0 + int(rng.integers(1, h + 1))], fill=tuple(int(v) for v in rng.integers(0, 256, 4)))
    d.line([0, 0, w, h], fill=(10, 20, 30, 200), width=2)
    return np.asarray(im)


def pillow_file(a: np.ndarray, mode: str, compression: str, predictor: bool) -> bytes:
    im = Image.fromarray(a).convert("RGB").quantize(200) if mode == "P" else Image.fromarray(a).convert(mode)
    b = io.BytesIO()
    im.save(b, "TIFF", compression=compression, **({"tiffinfo": {317: 2}} if predictor else {}))
    return b.getvalue()


SIZES = [(1, 1), (2, 3), (7, 5), (64, 64), (101, 77), (300, 200), (513, 517)]


def pillow_cases():
    """(name, file): L / RGB / RGBA / P x LZW / PackBits x predictor none / 2, 1 x 1 to past 512 x 512."""
    rng = np.random.default_rng(61)
    out = []
    for k, (w, h) in enumerate(SIZES):
        for j, mode in enumerate(("L", "RGB", "RGBA", "P")):
            a = content(rng, w, h, ("noise", "smooth", "drawing")[(k + j) % 3])
            for comp in ("tiff_lzw", "packbits"):
                for predictor in (False, True):
                    out.append((f"pillow_{mode}_{comp}_{'p2' if predictor else 'p1'}_{w}x{h}", pillow_file(a, mode, comp, predictor)))
    return out


def differenced(a: np.ndarray) -> np.ndarray:
    """Predictor 2, forward: every sample minus the one a pixel to its left, modulo 256."""
    b = a.reshape(a.shape[0], a.shape[1], -1).astype(np.int16)
    b[:, 1:] -= b[:, :-1].copy()
    return (b & 255).astype(np.uint8).reshape(a.shape)


def compressed(a: np.ndarray, comp: int, *, order="<", rows=None, predictor=None, long_fields=False, photo=None, extra=None, more=(), drop=(),
               encode=None, counts=None, sort=True) -> bytes:
    """A chunky 8-bit TIFF of ``a`` in strips of ``rows`` rows, each compressed on its own by ``encode`` (bytes -> bytes; default:
    the tests' plain LZW / PackBits writers).  ``drop``: tags left out; ``counts``: StripByteCounts values instead of the true ones."""
    h, w = a.shape[:2]
    spp = 1 if a.ndim == 2 else a.shape[2]
    rows = rows or h
    data = (differenced(a) if predictor == 2 else a).tobytes()
    stride = w * spp
    encode = encode or (Z.lzw if comp == LZW else Z.packbits)
    blobs, offs = [], []
    for s, y in enumerate(range(0, h, rows)):
        blobs.append((f"s{s}", encode(data[y * stride:(y + rows) * stride])))
        offs.append(("@", f"s{s}"))
    t = 4 if long_fields else 3
    photo = (2 if spp >= 3 else 1) if photo is None else photo
    entries = [(256, t, 1, [w]), (257, t, 1, [h]), (258, 3, spp, [8] * spp), (259, 3, 1, [comp]), (262, 3, 1, [photo]),
               (273, 4, len(offs), offs), (277, 3, 1, [spp]), (278, t, 1, [rows]),
               (279, t if max(len(b[1]) for b in blobs) < 65536 else 4, len(offs), counts or [len(b[1]) for b in blobs])]
    if predictor is not None:
        entries.append((317, 3, 1, [predictor]))
    if extra is not None:
        entries.append((338, 3, 1, [extra]))
    entries = [e for e in entries if e[0] not in drop] + list(more)
    if sort:
        entries.sort(key=lambda x: x[0])
    return T.tiff(entries, blobs, order=order)


def handmade_cases():
    """(name, file): both byte orders, SHORT and LONG fields, strips of 1 / 3 / H / more than H rows, every layout."""
    rng = np.random.default_rng(62)
    out = []
    for (w, h) in [(5, 4), (33, 17), (130, 41)]:
        g = content(rng, w, h, "smooth")[..., 0].copy()
        c3 = content(rng, w, h, "drawing")[..., :3].copy()
        c4 = content(rng, w, h, "noise")
        cmap = rng.integers(0, 65536, 768).tolist()
        for comp, cn in ((LZW, "lzw"), (PACKBITS, "packbits")):
            for order in "<>":
                o = f"{cn}_{'II' if order == '<' else 'MM'}_{w}x{h}"
                kw = dict(order=order)
                out += [(f"gray_{o}", compressed(g, comp, **kw)),
                        (f"gray_white_is_zero_{o}", compressed(g, comp, photo=0, **kw)),
                        (f"gray_p2_rows3_{o}", compressed(g, comp, predictor=2, rows=3, **kw)),
                        (f"rgb_{o}", compressed(c3, comp, **kw)),
                        (f"rgb_strips_of_1_{o}", compressed(c3, comp, rows=1, **kw)),
                        (f"rgb_strips_of_3_p2_{o}", compressed(c3, comp, rows=3, predictor=2, **kw)),
                        (f"rgb_long_fields_{o}", compressed(c3, comp, rows=2, long_fields=True, **kw)),
                        (f"rgb_rows_beyond_height_{o}", compressed(c3, comp, rows=h + 7, predictor=1, **kw)),
                        (f"rgba_unassociated_p2_{o}", compressed(c4, comp, extra=2, predictor=2, **kw)),
                        (f"rgba_no_extrasamples_{o}", compressed(c4, comp, rows=5, **kw)),
                        (f"rgbx_{o}", compressed(c4, comp, extra=0, rows=3, **kw)),
                        (f"rgbx_p2_{o}", compressed(c4, comp, extra=0, predictor=2, **kw)),
                        (f"palette_{o}", compressed(g, comp, photo=3, more=[(320, 3, 768, cmap)], **kw)),
                        (f"palette_p2_{o}", compressed(g, comp, photo=3, predictor=2, rows=4, more=[(320, 3, 768, cmap)], **kw)),
                        (f"gray_software_resolution_{o}", compressed(g, comp, more=[(282, 5, 1, [(72, 1)]), (283, 5, 1, [(72, 1)]), (296, 3, 1, [2]),
                                                                                  (305, 2, 12, b"made by hand")], **kw))]
    return out


def _run_heavy(rng, n: int) -> bytes:
    """Noise with runs of one byte in it: fills the table and meets the KwKwK case all the way."""
    out = bytearray()
    while len(out) < n:
        out += rng.integers(0, 256, int(rng.integers(20, 200)), dtype=np.uint8).tobytes()
        out += bytes([int(rng.integers(0, 256))]) * int(rng.integers(3, 40))
    return bytes(out[:n])


def lzw_stream_cases():
    """(name, file): valid streams libtiff's writer never produces, as gray files of one or a few strips."""
    rng = np.random.default_rng(63)
    w, h = 96, 80
    a = np.frombuffer(_run_heavy(rng, w * h), np.uint8).reshape(h, w)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    out = []
    assert Z.kwkwk_widths(Z.codes_of(a.tobytes())) == {9, 10, 11, 12}
    for name, how in [("plain", {}), ("clear_at_4095", dict(clear_at=4095)), ("clear_at_4096", dict(clear_at=4096)), ("clear_at_511", dict(clear_at=511)),
                      ("clear_at_512", dict(clear_at=512)), ("clear_at_1023", dict(clear_at=1023)), ("clear_at_1024", dict(clear_at=1024)), ("clear_at_2047", dict(clear_at=2047)),
                      ("clear_at_2048", dict(clear_at=2048)), ("clear_in_mid_strip", dict(clear_every=100)), ("clear_every_code", dict(clear_every=1)), ("no_eoi", dict(eoi=False))]:
        for src, sn in ((a, "runs"), (noise, "noise")):
            out.append((f"lzw_{name}_{sn}", compressed(src, LZW, encode=lambda d, how=how: Z.lzw(d, **how))))
    out.append(("lzw_bytes_after_eoi", compressed(a, LZW, rows=20, encode=lambda d: Z.lzw(d) + b"\x12\x34\x56\x78\x9a")))
    out.append(("lzw_no_eoi_then_junk", compressed(a, LZW, rows=20, encode=lambda d: Z.lzw(d + b"\x55" * 9, eoi=False))))
    out.append(("lzw_double_clear", compressed(a, LZW, encode=lambda d: Z.pack([Z.CLEAR] + Z.codes_of(d)))))
    out.append(("lzw_one_row_strips", compressed(a, LZW, rows=1)))
    out.append(("lzw_one_pixel_strips", compressed(a[:, :1].copy(), LZW, rows=1)))
    out.append(("lzw_one_pixel_strips_rgb_p2", compressed(np.ascontiguousarray(content(rng, 1, 9, "noise")[..., :3]), LZW, rows=1, predictor=2)))
    flat = np.full((300, 300), 7, np.uint8)                  # strings far longer than a copy record holds
    out.append(("lzw_flat", compressed(flat, LZW)))
    out.append(("lzw_flat_p2_rgb", compressed(np.full((200, 150, 3), 200, np.uint8), LZW, predictor=2, rows=64)))
    return out


def packbits_stream_cases():
    """(name, file): the hand-written corner cases."""
    rng = np.random.default_rng(64)
    out = []
    row = bytes(rng.integers(0, 256, 128, dtype=np.uint8))
    a = np.frombuffer(row * 4, np.uint8).reshape(4, 128)
    out.append(("packbits_128_byte_literals", compressed(a, PACKBITS, encode=lambda d: b"".join(bytes([127]) + d[k:k + 128] for k in range(0, len(d), 128)))))
    out.append(("packbits_noop_headers", compressed(a, PACKBITS, encode=lambda d: b"\x80" + b"".join(b"\x80" + bytes([127]) + d[k:k + 128] + b"\x80\x80" for k in range(0, len(d), 128)))))
    flat = np.full((6, 64), 99, np.uint8)                     # 384 bytes: three 128-byte runs, each crossing a row's end
    out.append(("packbits_128_byte_runs_crossing_rows", compressed(flat, PACKBITS, encode=lambda d: bytes([129, 99]) * (len(d) // 128))))
    b = np.frombuffer(bytes([5] * 100 + [6] * 92), np.uint8).reshape(3, 64)
    out.append(("packbits_runs_crossing_rows", compressed(b, PACKBITS, encode=lambda d: bytes([257 - 100, 5, 257 - 92, 6]))))
    out.append(("packbits_two_byte_runs", compressed(b, PACKBITS, encode=lambda d: b"".join(bytes([255, v]) for v in d[::2]))))
    out.append(("packbits_single_literals", compressed(a, PACKBITS, encode=lambda d: b"".join(bytes([0, v]) for v in d))))
    out.append(("packbits_run_cut_at_the_end", compressed(b, PACKBITS, encode=lambda d: bytes([257 - 100, 5, 257 - 128, 6]))))          # libtiff warns and clamps
    out.append(("packbits_literal_cut_at_the_end", compressed(a, PACKBITS, encode=lambda d: Z.packbits(d[:-3]) + bytes([9]) + d[-3:] + bytes(7))))
    out.append(("packbits_bytes_after_the_end", compressed(a, PACKBITS, rows=2, encode=lambda d: Z.packbits(d) + b"\x03abcd")))
    out.append(("packbits_one_pixel_strips", compressed(a[:, :1].copy(), PACKBITS, rows=1)))
    out.append(("packbits_rgb_p2_flat", compressed(np.full((40, 70, 3), 31, np.uint8), PACKBITS, predictor=2, rows=7)))
    return out


def sink_cases():
    """(name, file): the copy patterns of tests/_gif_stream_cases.py that stress the sink the two LZW walkers share and the
    copies at length bias 2 -- runs of every distance 2..17, at the start of the records and across a round of 64, and last
    strings cut to one byte -- as one-strip gray files."""
    import _gif_stream_cases as S

    return [(name, compressed(np.zeros((h, w), np.uint8), LZW, encode=lambda d, codes=codes: Z.pack(codes))) for name, w, h, codes in S.tiff_strips()]


def valid_cases():
    """Every file the decoder must take, (family, name, file)."""
    return ([("pillow", n, d) for n, d in pillow_cases()] + [("handmade", n, d) for n, d in handmade_cases()] +
            [("lzw_streams", n, d) for n, d in lzw_stream_cases()] + [("packbits_streams", n, d) for n, d in packbits_stream_cases()])


def refused_cases():
    """(name, file, status): 1 = left to Pillow, 2 = damaged (Pillow raises)."""
    rng = np.random.default_rng(65)
    c3 = np.ascontiguousarray(content(rng, 24, 18, "smooth")[..., :3])
    g = c3[..., 0].copy()
    good = compressed(c3, LZW, rows=4)
    n_strips = 5
    out = [("uncompressed", T.plain(c3, rows=4), 1),
           ("deflate", compressed(c3, 8, encode=lambda d: __import__("zlib").compress(d)), 1),
           ("deflate_old", compressed(c3, 32946, encode=lambda d: __import__("zlib").compress(d)), 1),
           ("jpeg_tag", compressed(c3, 7, encode=lambda d: d), 1),
           ("ccitt_tag", compressed(g, 4, encode=lambda d: d), 1),
           ("tiles", compressed(c3, LZW, more=[(322, 3, 1, [16]), (323, 3, 1, [16]), (324, 4, 1, [8]), (325, 4, 1, [100])]), 1),
           ("tile_width_alone", compressed(c3, LZW, more=[(322, 3, 1, [16])]), 1),
           ("planar", compressed(c3, LZW, more=[(284, 3, 1, [2])]), 1),
           ("bits_16", compressed(c3, LZW, drop=(258,), more=[(258, 3, 3, [16, 16, 16])]), 1),
           ("bits_one_value_for_three_samples", compressed(c3, LZW, drop=(258,), more=[(258, 3, 1, [8])]), 1),
           ("predictor_3", compressed(c3, LZW, predictor=3), 1),
           ("predictor_long", compressed(c3, LZW, more=[(317, 4, 1, [2])]), 1),
           ("predictor_two_values", compressed(c3, LZW, more=[(317, 3, 2, [2, 2])]), 1),
           ("no_strip_byte_counts", compressed(c3, LZW, rows=4, drop=(279,)), 1),
           ("short_strip_byte_counts", compressed(c3, LZW, rows=4, drop=(279,), more=[(279, 4, n_strips - 1, [40] * (n_strips - 1))]), 1),
           ("strip_byte_count_zero", compressed(c3, LZW, rows=4, counts=[0] * n_strips), 1),
           ("too_few_strips", compressed(c3, LZW, rows=4, drop=(257,), more=[(257, 3, 1, [30])]), 1),
           ("duplicate_width", compressed(c3, LZW, more=[(256, 3, 1, [24])]), 1),
           ("duplicate_software", compressed(c3, LZW, more=[(305, 2, 4, b"abc\0"), (305, 2, 4, b"abd\0")]), 1),
           ("descending_tags", compressed(c3, LZW, sort=False, more=[(254, 4, 1, [0])]), 1),
           ("unknown_tag", compressed(c3, LZW, more=[(65000, 3, 1, [7])]), 1),
           ("unknown_type", compressed(c3, LZW, more=[(305, 14, 1, [7])]), 1),
           ("orientation_6", compressed(c3, LZW, more=[(274, 3, 1, [6])]), 1),
           ("exif_ifd", compressed(c3, LZW, more=[(34665, 4, 1, [8])]), 1),
           ("xmp", compressed(c3, LZW, more=[(700, 1, 30, b'<x tiff:Orientation="6"></x>  ')]), 1),
           ("fill_order_2", compressed(c3, LZW, more=[(266, 3, 1, [2])]), 1),
           ("premultiplied_alpha", compressed(content(rng, 9, 7, "noise"), LZW, extra=1), 1),
           ("bigtiff", good[:2] + b"\x2b\x00" + good[4:], 1),
           ("not_tiff", b"IJ" + good[2:], 2),
           ("strip_leaves_the_file", compressed(c3, LZW, rows=4, counts=[len(good)] * n_strips), 2),
           ("file_cut_in_the_last_strip", _cut_in_last_strip(c3), 2)]
    # invalid streams
    data = c3.tobytes()
    body = Z.codes_of(data)
    out += [("lzw_no_opening_clear", compressed(c3, LZW, encode=lambda d: Z.pack(Z.codes_of(d, open_clear=False))), 1),
            ("lzw_old_style_opening", compressed(c3, LZW, encode=lambda d: Z.pack(Z.codes_of(d), lsb=True, early=False)), 1),
            ("lzw_table_full_without_clear", compressed(np.frombuffer(_run_heavy(rng, 120 * 100), np.uint8).reshape(100, 120), LZW,
                                                        encode=lambda d: Z.lzw(d, clear_at=None)), 1),
            ("lzw_code_beyond_the_table", compressed(c3, LZW, encode=lambda d: Z.pack(body[:40] + [500] + body[40:])), 2),
            ("lzw_code_beyond_the_table_after_clear", compressed(c3, LZW, encode=lambda d: Z.pack([Z.CLEAR, 300] + body[1:])), 2),
            ("lzw_early_eoi", compressed(c3, LZW, encode=lambda d: Z.pack(body[:100] + [Z.EOI])), 2),
            ("lzw_clear_then_eoi", compressed(c3, LZW, encode=lambda d: Z.pack(body[:100] + [Z.CLEAR, Z.EOI])), 2),
            ("lzw_short_strip", compressed(c3, LZW, encode=lambda d: Z.lzw(d[:-50], eoi=False)), 2),
            ("lzw_short_strip_with_eoi", compressed(c3, LZW, encode=lambda d: Z.lzw(d[:-1])), 2),
            ("packbits_short_strip", compressed(c3, PACKBITS, encode=lambda d: Z.packbits(d[:-1])), 2),
            ("packbits_literal_cut_by_the_bytes", compressed(c3, PACKBITS, encode=lambda d: Z.packbits(d[:-9]) + bytes([8]) + d[-9:-1]), 2),
            ("packbits_run_without_its_byte", compressed(c3, PACKBITS, encode=lambda d: Z.packbits(d[:-9]) + bytes([257 - 9])), 2)]
    return out


def _cut_in_last_strip(a):
    data = compressed(a, LZW, rows=4, more=[(305, 2, 8, b"abcdefg\0")])
    # the strips lie in front of the directory; a copy of the file with the directory moved in front of them would be another
    # file -- so: the last strip's offset pushed to the file's last bytes, its count unchanged
    ifd = struct.unpack("<I", data[4:8])[0]
    n = struct.unpack("<H", data[ifd:ifd + 2])[0]
    for k in range(n):
        e = ifd + 2 + 12 * k
        tag, typ, count, value = struct.unpack("<HHII", data[e:e + 12])
        if tag == 273:
            at = value + 4 * (count - 1)
            return data[:at] + struct.pack("<I", len(data) - 3) + data[at + 4:]
    raise AssertionError


def late_change_cases():
    """(name, file): valid data written with the "late change" width rule -- a libtiff-style reader reads other codes from the
    first width change on; whatever libtiff makes of them, the decoder makes the same or refuses."""
    rng = np.random.default_rng(66)
    out = []
    for k in range(6):
        a = np.frombuffer(_run_heavy(rng, 60 * 50), np.uint8).reshape(50, 60)
        out.append((f"lzw_late_change_{k}", compressed(a, LZW, rows=(None, 25, 10)[k % 3], encode=lambda d: Z.lzw(d, early=False))))
    return out


def fuzz_bases():
    """(compression, file): small files of every kind for the damage."""
    rng = np.random.default_rng(67)
    c3 = np.ascontiguousarray(content(rng, 40, 30, "smooth")[..., :3])
    d3 = np.ascontiguousarray(content(rng, 37, 29, "drawing")[..., :3])
    g = content(rng, 50, 40, "noise")[..., 0].copy()
    c4 = content(rng, 21, 33, "drawing")
    out = []
    for comp in (LZW, PACKBITS):
        out += [(comp, compressed(c3, comp, rows=8)), (comp, compressed(d3, comp, rows=5, predictor=2, order=">")), (comp, compressed(g, comp, rows=16)),
                (comp, compressed(c4, comp, extra=2, predictor=2)), (comp, compressed(d3[..., 0].copy(), comp, photo=0, rows=7, long_fields=True)),
                (comp, pillow_file(content(rng, 45, 35, "smooth"), "RGB", "tiff_lzw" if comp == LZW else "packbits", comp == LZW)),
                (comp, pillow_file(content(rng, 30, 30, "drawing"), "P", "tiff_lzw" if comp == LZW else "packbits", False))]
    return out


def _regions(data: bytes):
    """(directory range, strip ranges, positions of the StripByteCounts values with their sizes) of a well-formed file."""
    e = "<" if data[:2] == b"II" else ">"
    ifd = struct.unpack(e + "I", data[4:8])[0]
    n = struct.unpack(e + "H", data[ifd:ifd + 2])[0]
    tags = {}
    for k in range(n):
        at = ifd + 2 + 12 * k
        tag, typ, count = struct.unpack(e + "HHI", data[at:at + 8])
        size = {3: 2, 4: 4}.get(typ, 1) * count
        where = at + 8 if size <= 4 else struct.unpack(e + "I", data[at + 8:at + 12])[0]
        tags[tag] = (typ, count, where)
    def values(tag):
        typ, count, where = tags[tag]
        f, s = ("H", 2) if typ == 3 else ("I", 4)
        return [struct.unpack(e + f, data[where + s * k:where + s * k + s])[0] for k in range(count)], [(where + s * k, s) for k in range(count)]
    offs, _ = values(273)
    counts, count_at = values(279)
    return (ifd, ifd + 2 + 12 * n + 4), list(zip(offs, counts)), count_at, e


def damaged(base: bytes, rng, count: int):
    """``count`` damaged copies: directory bytes, strip bytes flipped / overwritten, the file cut, byte counts changed."""
    (d0, d1), strips, count_at, e = _regions(base)
    out = []
    for k in range(count):
        b = bytearray(base)
        how = k % 8
        if how == 0:                                                 # a directory byte
            b[int(rng.integers(d0, d1))] = int(rng.integers(0, 256))
        elif how in (1, 2):                                          # a bit of a strip
            off, n = strips[int(rng.integers(0, len(strips)))]
            b[off + int(rng.integers(0, n))] ^= 1 << int(rng.integers(0, 8))
        elif how == 3:                                               # a byte of a strip
            off, n = strips[int(rng.integers(0, len(strips)))]
            b[off + int(rng.integers(0, n))] = int(rng.integers(0, 256))
        elif how == 4:                                               # a stretch of a strip overwritten
            off, n = strips[int(rng.integers(0, len(strips)))]
            at = int(rng.integers(0, n))
            m = min(n - at, int(rng.integers(1, 12)))
            b[off + at:off + at + m] = rng.integers(0, 256, m, dtype=np.uint8).tobytes()
        elif how == 5:                                               # the file cut
            b = b[:int(rng.integers(8, len(b)))]
        elif how == 6:                                               # a byte count changed a little, or a lot
            at, s = count_at[int(rng.integers(0, len(count_at)))]
            v = int.from_bytes(b[at:at + s], "little" if e == "<" else "big")
            v = max(0, v + int(rng.integers(-6, 7))) if k % 16 == 6 else int(rng.integers(0, 1 << (8 * s)))
            b[at:at + s] = (v % (1 << (8 * s))).to_bytes(s, "little" if e == "<" else "big")
        else:                                                        # any byte at all
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        out.append(bytes(b))
    return out


def damaged_set(per_base: int = 400, seed: int = 2026):
    """The damaged files of the census, [(compression, file)]: 14 bases x 400, the same on the CPU and through the kernels."""
    rng = np.random.default_rng(seed)
    return [(comp, data) for comp, base in fuzz_bases() for data in damaged(base, rng, per_base)]
