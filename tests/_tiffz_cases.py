"""Deflate-compressed TIFF files for the decoder tests (ke_tiffz_*): what Pillow / libtiff write with Compression 8 ("Adobe
deflate") and its old alias 32946, with and without the horizontal predictor; hand-made directories (tests/_tiffc_cases.compressed)
around strips from zlib and from the tests' own deflate writer (tests/_deflate_write.py) for what no compressor writes; what
libtiff does with odd strips, each row with the decoder's status; the files that must be refused; and damage."""
from __future__ import annotations

import struct
import zlib

import numpy as np

import _deflate_write as D
import _tiffc_cases as A
from _tiffc_cases import CORRUPT, OK, UNSUPPORTED, compressed, content, pillow_file, pillow_pixels  # noqa: F401

DEFLATE, DEFLATE_OLD = 8, 32946
COMPRESSIONS = ((DEFLATE, "adobe"), (DEFLATE_OLD, "old"))


def pillow_cases():
    """(name, file): L / RGB / RGBA / P x tiff_adobe_deflate / tiff_deflate x predictor none / 2, 1 x 1 to past 512 x 512."""
    rng = np.random.default_rng(71)
    out = []
    for k, (w, h) in enumerate(A.SIZES):
        for j, mode in enumerate(("L", "RGB", "RGBA", "P")):
            a = content(rng, w, h, ("noise", "smooth", "drawing")[(k + j) % 3])
            for comp in ("tiff_adobe_deflate", "tiff_deflate"):
                for predictor in (False, True):
                    out.append((f"pillow_{mode}_{comp}_{'p2' if predictor else 'p1'}_{w}x{h}", pillow_file(a, mode, comp, predictor)))
    return out


def handmade_cases():
    """(name, file): both byte orders, SHORT and LONG fields, strips of 1 / 3 / H / more than H rows, every layout, both
    compression values; the strips are zlib's at changing levels."""
    rng = np.random.default_rng(72)
    out = []
    for (w, h) in [(5, 4), (33, 17), (130, 41)]:
        g = content(rng, w, h, "smooth")[..., 0].copy()
        c3 = content(rng, w, h, "drawing")[..., :3].copy()
        c4 = content(rng, w, h, "noise")
        cmap = rng.integers(0, 65536, 768).tolist()
        for comp, cn in COMPRESSIONS:
            for order in "<>":
                o = f"{cn}_{'II' if order == '<' else 'MM'}_{w}x{h}"
                kw = dict(order=order, encode=lambda d, level=(1, 6, 9)[(w + comp) % 3]: zlib.compress(d, level))
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


def _gray(raw: bytes):
    """The bytes as a gray image of one strip: the widest rows that divide them (a TIFF row has at most 65 535 pixels)."""
    n = len(raw)
    w = next((w for w in range(min(n, 65535), 0, -1) if n % w == 0))
    return np.frombuffer(raw, np.uint8).reshape(n // w, w)


def _strip_file(blocks, comp: int = DEFLATE, shape=None, **wrap) -> bytes:
    """A one-strip gray file whose strip is exactly these deflate blocks in a zlib wrapper."""
    s = D.Stream(blocks)
    assert s.raw is not None and zlib.decompress(D.zlib_wrap(s.bits, s.raw, **wrap)) == s.raw       # the installed zlib is the writer's check
    a = _gray(s.raw) if shape is None else np.frombuffer(s.raw, np.uint8).reshape(shape)
    return compressed(a, comp, long_fields=a.shape[0] > 65535, encode=lambda d: D.zlib_wrap(s.bits, s.raw, **wrap))


def _literals(rng, n: int, top: int = 256) -> list:
    return [int(v) for v in rng.integers(0, top, n)]


def named_stream_cases():
    """(name, file): the streams no compressor writes, by name, as one-strip gray files."""
    rng = np.random.default_rng(73)
    out = []
    # a 15-bit code in both alphabets
    ll = [0] * 258
    for v in range(13):
        ll[v] = v + 1
    ll[13] = ll[14] = ll[256] = ll[257] = 15
    dd = [k + 1 for k in range(14)] + [15, 15]
    t = _literals(rng, 400, 15)
    for ds in range(16):
        t += [(3, D.DIST_BASE[ds])] + _literals(rng, 2, 15)
    out.append(("code_of_15_bits", _strip_file([D.dynamic(t, ll, dd, final=True)])))
    # a distance tree of a single code
    t = _literals(rng, 30, 3) + [(10, 1)] + _literals(rng, 3, 3) + [(4, 1)] + _literals(rng, 2, 3)
    out.append(("single_code_distance_tree", _strip_file([D.auto_dynamic(t, final=True)], comp=DEFLATE_OLD)))
    # every block type behind every bit offset
    blocks = [D.fixed(_literals(rng, 1))]
    for k in range(60):
        lits = [200] * (k // 2 % 8) + _literals(rng, int(rng.integers(1, 4)), 144)       # 9-bit codes shift the end by one bit each
        data = rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8).tobytes()
        blocks += [D.fixed(lits) if k % 2 else D.auto_dynamic(lits, rng=rng), D.stored(data)]
    blocks[-1]["final"] = True
    s = D.Stream(blocks)
    assert all(s.census[f"stored_behind_bit_{b}"] for b in range(8)), s.census
    out.append(("every_block_type_behind_every_bit_offset", _strip_file(blocks)))
    # an empty stored block (and one of every type in front)
    t = _literals(rng, 50)
    out.append(("empty_stored_block", _strip_file([D.stored(b""), D.fixed([]), D.dynamic([], D.flat_lengths([256], 257), [0]), D.stored(b""),
                                                   D.fixed(t), D.stored(b"", final=True)])))
    # a match of 258 at distance 1, in both spellings
    out.append(("match_of_258_at_distance_1", _strip_file([D.fixed([77, (258, 1), 3, (258, 1, "284+31"), 9], final=True)])))
    # a match at distance 32 768: 331 x 100 gray, 33 100 bytes in one strip
    t = _literals(rng, 32768) + [(258, 32768), 5, (3, 32768), (40, 32767)]
    t += _literals(rng, 33100 - (32768 + 258 + 1 + 3 + 40))
    out.append(("match_at_distance_32768", _strip_file([D.auto_dynamic(t, final=True)], shape=(100, 331))))
    # a chain of 100 dependent copies: every copy reads what the copy in front of it wrote, too far back to be a run
    t = _literals(rng, 64)
    for k in range(100 + 1):
        t.append((20, 20 + k % 7))
    assert D.copy_census(t)["chain_of_100_dependent_copies"]
    out.append(("chain_of_100_dependent_copies", _strip_file([D.auto_dynamic(t, final=True)])))
    # the strip's length modulo 4, ending in a literal and ending in a copy
    for want in (61, 62, 63, 64):
        out.append((f"want_mod_4_is_{want % 4}_ends_in_literal", _strip_file([D.fixed(_literals(rng, 20) + [(want - 23, 7)] + _literals(rng, 3), final=True)])))
        out.append((f"want_mod_4_is_{want % 4}_ends_in_copy", _strip_file([D.fixed(_literals(rng, 20) + [(want - 20, 20)], final=True)], comp=DEFLATE_OLD)))
    return out


def png_stream_cases():
    """(name, file): every hand-written valid stream of the PNG inflate's tests (tests/_png_cases._valid_streams: codes, headers,
    copies of every length and distance, runs, chains, the zlib header's fields) as a one-strip gray file -- the same inflate,
    one lane per strip.  Left out: the streams that reach beyond the
    window their header declares (zlib inflates them; what libtiff's own zlib build does with them is not this module's to pin)."""
    import _png_cases as P

    out = []
    for k, (name, blocks, extra, wrap) in enumerate(P._valid_streams()):
        if D.Stream(blocks).raw is None or "distance_beyond_the_declared_window" in extra:
            continue
        wrap = {key: v for key, v in wrap.items() if key in ("cinfo", "flevel")}
        out.append((f"png_{name}", _strip_file(blocks, comp=COMPRESSIONS[k % 2][0], **wrap)))
    return out


def _encoders():
    """name -> (strip bytes -> stream, status, Pillow opens the file): what libtiff does with odd strips."""
    def fixed(d):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
        return c.compress(d) + c.flush()

    def flushed(d):
        c = zlib.compressobj(6)
        out = b""
        for k in range(0, len(d), max(1, len(d) // 4)):
            out += c.compress(d[k:k + max(1, len(d) // 4)]) + c.flush(zlib.Z_FULL_FLUSH)
        return out + c.flush()

    def window_512(d):
        c = zlib.compressobj(6, zlib.DEFLATED, 9)
        return c.compress(d) + c.flush()

    def raw_deflate(d):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        return c.compress(d) + c.flush()

    def gzip(d):
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        return c.compress(d) + c.flush()

    def preset(d):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, d[:16] or b"x")
        return c.compress(d) + c.flush()

    return {"stored_only": (lambda d: zlib.compress(d, 0), OK, True),
            "fixed_codes": (fixed, OK, True),
            "full_flushes_between_blocks": (flushed, OK, True),
            "window_of_512_bytes": (window_512, OK, True),
            "garbage_after_the_stream": (lambda d: zlib.compress(d) + b"\x01\x23\x45\x67\x89\xab\xcd", OK, True),
            "too_long": (lambda d: zlib.compress(d + b"abc"), CORRUPT, True),
            "cut_by_1": (lambda d: zlib.compress(d)[:-1], CORRUPT, True),
            "cut_by_4": (lambda d: zlib.compress(d)[:-4], CORRUPT, True),
            "wrong_trailer": (lambda d: zlib.compress(d)[:-1] + bytes([zlib.compress(d)[-1] ^ 1]), CORRUPT, False),
            "too_short": (lambda d: zlib.compress(d[:-3]), CORRUPT, False),
            "raw_deflate": (raw_deflate, CORRUPT, False),
            "gzip_wrapper": (gzip, CORRUPT, False),
            "preset_dictionary": (preset, CORRUPT, False)}


# The refusals Pillow does not share (libtiff stops inflating when the strip is full, so it never looks at what follows): the
# decoder wants one complete zlib stream per strip that yields exactly the strip's bytes.
STRICTER_THAN_LIBTIFF = ("too_long", "cut_by_1", "cut_by_4")


def odd_strip_cases():
    """(name, file, status, Pillow opens it): 33 x 17 RGB, one strip and strips of 5 rows, both compression values."""
    rng = np.random.default_rng(74)
    a = np.ascontiguousarray(content(rng, 33, 17, "smooth")[..., :3])
    out = []
    for name, (encode, status, opens) in _encoders().items():
        for comp, cn in COMPRESSIONS:
            for rows in (None, 5):
                out.append((f"{name}_{cn}_{'one_strip' if rows is None else 'strips_of_5'}", compressed(a, comp, rows=rows, encode=encode), status, opens))
    return out


def with_compression(data: bytes, comp: int) -> bytes:
    """The file with the value of its Compression tag (a SHORT in place) rewritten."""
    e = ">" if data[:2] == b"MM" else "<"
    ifd = struct.unpack(e + "I", data[4:8])[0]
    n = struct.unpack(e + "H", data[ifd:ifd + 2])[0]
    for k in range(n):
        at = ifd + 2 + 12 * k
        tag, typ, count = struct.unpack(e + "HHI", data[at:at + 8])
        if tag == 259 and typ == 3 and count == 1:
            return data[:at + 8] + struct.pack(e + "H", comp) + data[at + 10:]
    return data


def refused_cases():
    """(name, file, status): the refused set of tests/_tiffc_cases.py with Compression 5 rewritten to 8 -- the directory decides
    before any stream is looked at --, without the cases about LZW and PackBits streams and the two deflate files, which are
    this decoder's; and the other compressions."""
    out = []
    for name, data, status in A.refused_cases():
        if name.startswith(("lzw_", "packbits_")) or name in ("deflate", "deflate_old"):
            continue
        keeps = name in ("uncompressed", "jpeg_tag", "ccitt_tag")                # these are about their own Compression value
        rewritten = data if keeps else with_compression(data, DEFLATE)
        assert keeps or rewritten != data, name
        out.append((name, rewritten, status))
    rng = np.random.default_rng(75)
    c3 = np.ascontiguousarray(content(rng, 24, 18, "smooth")[..., :3])
    out += [("lzw", compressed(c3, A.LZW, rows=4), 1), ("packbits", compressed(c3, A.PACKBITS, rows=4), 1),
            ("zstd_tag", compressed(c3, 50000, encode=zlib.compress), 1), ("lzma_tag", compressed(c3, 34925, encode=zlib.compress), 1),
            ("predictor_3_deflate", compressed(c3, DEFLATE, predictor=3, encode=zlib.compress), 1),
            ("orientation_6_deflate", compressed(c3, DEFLATE, encode=zlib.compress, more=[(274, 3, 1, [6])]), 1),
            ("unknown_tag_deflate", compressed(c3, DEFLATE_OLD, encode=zlib.compress, more=[(65000, 3, 1, [7])]), 1),
            ("strip_byte_count_zero_deflate", compressed(c3, DEFLATE, rows=4, encode=zlib.compress, counts=[0] * 5), 1)]
    return out


def valid_cases():
    """Every file the decoder must take, (family, name, file)."""
    return ([("pillow", n, d) for n, d in pillow_cases()] + [("handmade", n, d) for n, d in handmade_cases()] +
            [("named_streams", n, d) for n, d in named_stream_cases()] + [("png_streams", n, d) for n, d in png_stream_cases()] +
            [("odd_strips", n, d) for n, d, st, _ in odd_strip_cases() if st == OK])


def corrupt_cases():
    """(name, file, Pillow opens it): every file whose status is 2."""
    return ([(n, d, opens) for n, d, st, opens in odd_strip_cases() if st == CORRUPT] +
            [(n, d, False) for n, d, st in refused_cases() if st == CORRUPT])


def fuzz_bases():
    """Small files of every kind for the damage."""
    rng = np.random.default_rng(77)
    c3 = np.ascontiguousarray(content(rng, 40, 30, "smooth")[..., :3])
    d3 = np.ascontiguousarray(content(rng, 37, 29, "drawing")[..., :3])
    g = content(rng, 50, 40, "noise")[..., 0].copy()
    c4 = content(rng, 21, 33, "drawing")
    z = zlib.compress
    return [compressed(c3, DEFLATE, rows=8, encode=z), compressed(d3, DEFLATE_OLD, rows=5, predictor=2, order=">", encode=z),
            compressed(g, DEFLATE, rows=16, encode=lambda d: z(d, 0)), compressed(c4, DEFLATE, extra=2, predictor=2, encode=z),
            compressed(d3[..., 0].copy(), DEFLATE_OLD, photo=0, rows=7, long_fields=True, encode=z),
            pillow_file(content(rng, 45, 35, "smooth"), "RGB", "tiff_adobe_deflate", True),
            pillow_file(content(rng, 30, 30, "drawing"), "P", "tiff_deflate", False),
            pillow_file(content(rng, 64, 48, "noise"), "L", "tiff_adobe_deflate", False)]


def damaged(base: bytes, rng, count: int):
    """``count`` damaged copies: tests/_tiffc_cases.damaged (directory and header bytes, strip bits / bytes / stretches, cuts, byte
    counts) and, every fifth, bytes inserted into a strip (what lies behind them in the strip moves back, its last bytes go)."""
    _, strips, _, _ = A._regions(base)
    out = A.damaged(base, rng, count)
    for k in range(4, count, 5):
        b = bytearray(base)
        off, n = strips[int(rng.integers(0, len(strips)))]
        m = min(n, int(rng.integers(1, 9)))
        at = int(rng.integers(0, n - m + 1))
        b[off + at:off + n] = rng.integers(0, 256, m, dtype=np.uint8).tobytes() + bytes(b[off + at:off + n - m])
        out[k] = bytes(b)
    return out


def damaged_set(per_base: int = 300, seed: int = 2027):
    """The damaged files of the census: 8 bases x 300, the same on the CPU and through the kernels."""
    rng = np.random.default_rng(seed)
    return [data for base in fuzz_bases() for data in damaged(base, rng, per_base)]
