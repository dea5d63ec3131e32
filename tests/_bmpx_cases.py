"""BMP files for the tests of the decoder of RLE, 1 / 4-bit and 16-bit files (ke_bmpx_*): Pillow cannot write them, so they come
from tests/_bmpx_write.py -- a grid of sizes for every kind, every 16-bit value, palettes of every length, every header variation
the parser reads, RLE streams written code by code for each rule of Pillow's BmpRleDecoder, random streams, real pictures through
the greedy encoder -- and the refusals with their status.  Pillow decides what the pixels are."""
from __future__ import annotations

import functools
import io

import numpy as np
from PIL import Image, ImageFile

import _bmpx_write as Wr
from _bmpx_write import EOB, EOL, Stream, delta, run
from _tiffc_cases import content

OK, UNSUPPORTED, CORRUPT = 0, 1, 2
KINDS = ("rle8", "rle4", "p1", "p4", "rgb555", "rgb555m", "rgb565")
M555, M565 = (0x7C00, 0x3E0, 0x1F), (0xF800, 0x7E0, 0x1F)


def pillow_pixels(data: bytes):
    """What the reference's hashes see of the file, strictly (a truncated file raises): palette / gray / two-colour files through
    convert("L"), 16-bit files as RGB.  None where Pillow raises."""
    was = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = False
    try:
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            return np.asarray(im.convert("L") if im.mode in ("P", "L", "1") else im)
    except Exception:
        return None
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = was


def palette(rng, n: int) -> bytes:
    """n entries of B, G, R, X -- never Pillow's gray identity (entry 0 is not black)."""
    p = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    p[0, :3] = (7, 99, 201)
    return p.tobytes()


GRAY256 = b"".join(bytes([v, v, v, 0]) for v in range(256))


def picture(kind: str, px: np.ndarray, *, pal: bytes = b"", colors=None, hs=40, topdown=False, gap=0, offset=None) -> bytes:
    """A file of ``kind`` around H x W indices (palette kinds; RLE through the greedy encoder) or H x W uint16 pixels."""
    n = len(pal) // 4
    colors = n if colors is None else colors
    if kind in ("rle8", "rle4"):
        comp = 1 if kind == "rle8" else 2
        data = Wr.encode_rle(px, Wr.data_start(hs, comp, n, gap), kind == "rle4", topdown)
        return Wr.bmp(px.shape[1], px.shape[0], 8 if kind == "rle8" else 4, data, hs=hs, comp=comp, colors=colors, palette=pal, topdown=topdown,
                      gap=gap, offset=offset)
    if kind in ("p1", "p4"):
        data = (Wr.rows1 if kind == "p1" else Wr.rows4)(px, topdown)
        return Wr.bmp(px.shape[1], px.shape[0], 1 if kind == "p1" else 4, data, hs=hs, colors=colors, palette=pal, topdown=topdown, gap=gap, offset=offset)
    comp, masks = {"rgb555": (0, ()), "rgb555m": (3, M555), "rgb565": (3, M565)}[kind]
    return Wr.bmp(px.shape[1], px.shape[0], 16, Wr.rows16(px, topdown), hs=hs, comp=comp, masks=masks, topdown=topdown, gap=gap, offset=offset)


def _indices(rng, kind: str, w: int, h: int, top: int = 0) -> np.ndarray:
    if kind in ("rgb555", "rgb555m", "rgb565"):
        return rng.integers(0, 65536, (h, w)).astype(np.uint16)
    top = top or {"rle8": 256, "rle4": 16, "p1": 2, "p4": 16}[kind]
    a = rng.integers(0, top, (h, w)).astype(np.uint8)
    if kind in ("rle8", "rle4") and w > 4:                 # some flat stretches, so that the encoder writes runs as well
        a[:, w // 3:w // 3 + max(3, w // 2)] = a[:, w // 3:w // 3 + 1]
    return a


def _ncolors(kind: str) -> int:
    return {"rle8": 256, "rle4": 16, "p1": 2, "p4": 16}.get(kind, 0)


def rle_file(w: int, h: int, stream: bytes, *, rle4=False, pal=None, colors=None, hs=40, topdown=False, gap=0, offset=None) -> bytes:
    """An RLE file around a stream written by hand; the default palette has 256 / 16 colours (see ``palette``)."""
    pal = palette(np.random.default_rng(w * 131 + h), 16 if rle4 else 256) if pal is None else pal
    return Wr.bmp(w, h, 4 if rle4 else 8, stream, hs=hs, comp=2 if rle4 else 1, colors=len(pal) // 4 if colors is None else colors, palette=pal,
                  topdown=topdown, gap=gap, offset=offset)


def _start(rle4: bool, gap: int = 0) -> int:
    return Wr.data_start(40, 2 if rle4 else 1, 16 if rle4 else 256, gap)


def handwritten_rle():
    """[(name, file, features)]: one stream per rule of BmpRleDecoder.decode, for RLE8 and RLE4, valid (Pillow opens every one)."""
    out = []
    for rle4 in (False, True):
        t = "rle4" if rle4 else "rle8"
        v = (lambda a, b=None: (a << 4) | (a if b is None else b)) if rle4 else (lambda a, b=None: a)

        def add(name, w, h, s, feats, **kw):
            out.append((f"{t}_{name}", rle_file(w, h, s.bytes() if isinstance(s, Stream) else s, rle4=rle4, **kw), set(feats)))

        for n in (1, 2, 254, 255):
            add(f"run_of_{n}", n, 2, run(n, v(3, 5)) + EOL + run(n, v(9)) + EOB, {f"run_{n}"})
        for gap in (0, 1):
            for n in (3, 4, 254, 255):
                s = Stream(_start(rle4, gap), rle4).absolute([(k * 7 + 1) % 16 for k in range(n)]).add(run(1, v(2)) + EOL).add(run(n, v(6)) + EOB)
                add(f"absolute_of_{n}_offset_parity_{gap}", n, 2, s, {f"absolute_{n}", f"parity_{gap}"}, gap=gap)
        if rle4:
            for n in range(3, 10):                         # an odd n yields n - 1 pixels while x += n
                s = Stream(_start(True), True).absolute([(k + 1) % 16 for k in range(n)]).add(run(12, 0x4A) + EOL + run(12, 0x11) + EOB)
                add(f"absolute_every_n_{n}", 12, 2, s, {f"rle4_absolute_{n}"})
        add("run_clipped_at_row_end_and_runs_after_it", 5, 2, run(3, v(1)) + run(9, v(2, 7)) + run(4, v(3)) + run(1, v(4)) + EOL + run(5, v(5)) + EOB,
            {"run_clipped", "runs_after_clip"})
        s = Stream(_start(rle4), rle4).add(run(2, v(1))).absolute([1, 2, 3, 4, 5, 6]).add(run(2, v(9)) + EOL).add(run(4, v(8)) + EOL + run(4, v(7)) + EOB)
        add("absolute_spills_into_next_row", 4, 3, s, {"absolute_spill"})
        s = Stream(_start(rle4), rle4).add(run(4, v(7)) + EOL).absolute([1, 2, 3, 4, 5, 6])
        add("absolute_spills_past_last_row", 4, 2, s, {"absolute_spill_past_end"})
        add("eol_on_full_and_partial_row", 4, 3, run(4, v(1)) + EOL + run(2, v(2)) + EOL + EOL + run(4, v(3)) + EOB, {"eol_full_row", "eol_partial_row"})
        add("delta_0_0", 4, 2, run(2, v(1)) + delta(0, 0) + run(2, v(2)) + EOL + run(4, v(3)) + EOB, {"delta_0_0"})
        add("delta_right", 6, 2, run(1, v(1)) + delta(3, 0) + run(2, v(2)) + EOL + run(6, v(3)) + EOB, {"delta_right"})
        add("delta_up", 4, 3, run(1, v(1)) + delta(0, 1) + run(3, v(2)) + EOL + run(4, v(3)) + EOB, {"delta_up"})
        add("delta_255_255", 300, 258, run(2, v(1)) + delta(255, 255) + run(40, v(2)) + EOL + run(255, v(3)) + run(45, v(4)) + EOL +
            delta(0, 255) + EOB, {"delta_255_255"})
        add("delta_past_the_end", 4, 3, run(4, v(5)) + EOL + run(1, v(6)) + delta(2, 9), {"delta_past_end"})
        add("delta_then_run_clipped_by_new_x", 5, 2, run(4, v(1)) + delta(3, 0) + run(5, v(2)) + EOL + run(3, v(3)) + EOB, {"delta_sets_x"})
        add("end_of_bitmap_exactly_when_full", 3, 2, run(3, v(1)) + EOL + run(3, v(2)) + EOB, {"eob_when_full"})
        # (a second run of W in the same row would be cut to nothing: x is reset by end-of-line and delta only)
        add("complete_without_any_eol", 4, 1, run(4, v(1, 2)), {"no_eol"})
        s = Stream(_start(rle4), rle4).absolute([1, 2, 3, 4]).absolute([5, 6, 7, 8]).absolute([9, 10, 11, 12])
        add("complete_without_any_eol_by_absolute_runs", 4, 3, s, {"no_eol"})
        add("complete_without_any_eol_by_deltas", 4, 3, run(4, v(1)) + delta(0, 0) + run(4, v(2)) + delta(0, 0) + run(4, v(3)), {"no_eol"})
        add("bytes_behind_a_full_picture", 4, 2, run(4, v(1)) + EOL + run(4, v(2)) + EOL + run(4, v(3)) + b"\x00", {"trailing_bytes"})
        add("topdown_stream", 4, 3, run(4, v(1)) + EOL + run(2, v(2)) + EOL + run(3, v(3)) + EOL, {"handwritten_topdown"}, topdown=True)
        add("stream_by_offset_0", 4, 2, run(4, v(1)) + EOL + run(4, v(2)) + EOB, {"handwritten_offset_0"}, offset=0)
    # the issue's example: bytes beyond W * H are dropped -- rows 1 2 3 4 / 7 7 7 7
    s = Stream(_start(False), False).add(run(4, 7) + EOL).absolute([1, 2, 3, 4, 5, 6])
    out.append(("rle8_example_rows_1234_7777", rle_file(4, 2, s.bytes(), pal=GRAY256), {"example_gray"}))
    return out


@functools.lru_cache(maxsize=None)
def valid_cases():
    """[(name, file, features)] -- every file is one Pillow opens and the decoder must take (tests/test_bmpx_cpu.py asserts both)."""
    rng = np.random.default_rng(2027)
    out = []
    for kind in KINDS:
        pal = palette(rng, _ncolors(kind)) if _ncolors(kind) else b""
        for w in list(range(1, 18)) + [31, 32, 33]:
            for h in (1, 2, 3):
                out.append((f"{kind}_{w}x{h}", picture(kind, _indices(rng, kind, w, h), pal=pal), {f"grid_{kind}"}))
        px = _indices(rng, kind, 13, 7)
        out.append((f"{kind}_topdown", picture(kind, px, pal=pal, topdown=True), {f"topdown_{kind}"}))
        out.append((f"{kind}_hs124", picture(kind, px, pal=pal, hs=124), {"hs_124", f"hs124_{kind}"}))
        out.append((f"{kind}_hs124_topdown", picture(kind, px, pal=pal, hs=124, topdown=True), {f"topdown_{kind}"}))
        out.append((f"{kind}_odd_data_offset", picture(kind, px, pal=pal, gap=1), {"offset_odd", f"offset_odd_{kind}"}))
        out.append((f"{kind}_gap_2", picture(kind, px, pal=pal, gap=2), {"offset_even"}))
        out.append((f"{kind}_data_offset_0", picture(kind, px, pal=pal, offset=0), {"offset_0", f"offset0_{kind}"}))
        if pal:
            out.append((f"{kind}_offset_at_palette", picture(kind, px, pal=pal, offset=54), {"offset_at_palette"}))
            out.append((f"{kind}_colors_field_0", picture(kind, px, pal=pal, colors=0), {"colors_0_palette"}))
    for kind in ("rgb555", "rgb555m", "rgb565"):
        every = np.arange(65536, dtype=np.uint32).reshape(256, 256).astype(np.uint16)
        out.append((f"{kind}_every_value", picture(kind, every), {f"every_value_{kind}"}))
        out.append((f"{kind}_every_value_hs124", picture(kind, every[::-1].copy(), hs=124, topdown=True), {f"every_value_{kind}"}))
    # Pillow's raw decoder does not ask for the padding behind the last stored row
    out.append(("p4_last_rows_padding_missing", picture("p4", _indices(rng, "p4", 11, 4), pal=palette(rng, 16))[:-2], {"padding_missing"}))
    out.append(("p1_last_rows_padding_missing", picture("p1", _indices(rng, "p1", 33, 4), pal=palette(rng, 2))[:-3], {"padding_missing"}))
    out.append(("rgb565_last_rows_padding_missing", picture("rgb565", _indices(rng, "rgb565", 11, 4), topdown=True)[:-2], {"padding_missing"}))
    out.append(("rgb555_colors_field_0", picture("rgb555", _indices(rng, "rgb555", 9, 4), colors=0), {"colors_0_16bit"}))
    # palettes of every length; the indices run beyond a short one (black in mode P)
    for n in (1, 2, 3, 15, 16, 17, 255, 256):
        pal = palette(rng, n)
        for kind in ("rle8", "rle4", "p4", "p1"):
            px = _indices(rng, kind, 21, 5)
            beyond = n < {"rle8": 256, "rle4": 16, "p4": 16, "p1": 2}[kind]
            out.append((f"{kind}_palette_of_{n}", picture(kind, px, pal=pal), {f"palette_{n}"} | ({"index_beyond_palette"} if beyond else set())))
    # gray-identity palettes: mode L, the indices pass through -- also beyond a short one
    out.append(("rle8_gray_256", picture("rle8", _indices(rng, "rle8", 19, 6), pal=GRAY256), {"gray_rle8"}))
    out.append(("rle8_gray_16_indices_beyond", picture("rle8", _indices(rng, "rle8", 19, 6), pal=GRAY256[:64]), {"gray_rle8", "gray_short"}))
    out.append(("rle4_gray_16", picture("rle4", _indices(rng, "rle4", 19, 6), pal=GRAY256[:64]), {"gray_rle4"}))
    out.append(("rle4_gray_3_indices_beyond", picture("rle4", _indices(rng, "rle4", 19, 6), pal=GRAY256[:12]), {"gray_rle4", "gray_short"}))
    bw, wb = bytes([0, 0, 0, 0, 255, 255, 255, 0]), bytes([255, 255, 255, 0, 0, 0, 0, 0])
    for w, h in ((1, 1), (9, 3), (33, 5), (64, 2)):
        px = _indices(rng, "p1", w, h)
        out.append((f"p1_black_white_{w}x{h}", picture("p1", px, pal=bw), {"p1_black_white"}))
        out.append((f"p1_white_black_{w}x{h}", picture("p1", px, pal=wb), {"p1_white_black"}))
    out.append(("p1_black_white_topdown", picture("p1", _indices(rng, "p1", 17, 4), pal=bw, topdown=True), {"p1_black_white"}))
    out.append(("rle8_two_colours_white_black", picture("rle8", _indices(rng, "rle8", 9, 3, 2), pal=wb), {"rle_two_colours"}))
    out += handwritten_rle()
    # real pictures at 64 x 48 through the greedy encoder, with the palettes Pillow's quantiser finds
    for k, what in enumerate(("drawing", "smooth", "noise", "drawing")):
        rgb = Image.fromarray(np.ascontiguousarray(content(rng, 64, 48, what)[..., :3]))
        for kind, n in (("rle8", 256), ("rle4", 16), ("p4", 16), ("p1", 2)):
            q = rgb.quantize(n)
            pal = np.asarray(q.getpalette()[:3 * n], np.uint8).reshape(-1, 3)
            pal = np.concatenate([pal[:, ::-1], np.zeros((len(pal), 1), np.uint8)], 1)
            if n == 2:
                pal[0, :3] = (12, 40, 90)                  # (never black then white: that is another case)
            out.append((f"{kind}_picture_{what}_{k}", picture(kind, np.asarray(q), pal=pal.tobytes(), topdown=k == 3), {"real_picture", f"picture_{kind}"}))
        px = np.asarray(rgb).astype(np.uint16)
        out.append((f"rgb565_picture_{what}_{k}", picture("rgb565", (px[..., 0] >> 3 << 11) | (px[..., 1] >> 2 << 5) | (px[..., 2] >> 3)),
                    {"real_picture", "picture_rgb565"}))
    return out


FEATURES = (
    [f"grid_{k}" for k in KINDS] + [f"topdown_{k}" for k in KINDS] + [f"hs124_{k}" for k in KINDS] + [f"offset_odd_{k}" for k in KINDS] +
    [f"offset0_{k}" for k in KINDS] + [f"every_value_{k}" for k in ("rgb555", "rgb555m", "rgb565")] + [f"palette_{n}" for n in (1, 2, 3, 15, 16, 17, 255, 256)] +
    ["index_beyond_palette", "gray_rle8", "gray_rle4", "gray_short", "p1_black_white", "p1_white_black", "offset_even", "offset_at_palette",
     "colors_0_palette", "colors_0_16bit", "padding_missing", "rle_two_colours", "run_1", "run_2", "run_254", "run_255", "absolute_3", "absolute_4", "absolute_254",
     "absolute_255", "parity_0", "parity_1"] + [f"rle4_absolute_{n}" for n in range(3, 10)] +
    ["run_clipped", "runs_after_clip", "absolute_spill", "absolute_spill_past_end", "eol_full_row", "eol_partial_row", "delta_0_0", "delta_right",
     "delta_up", "delta_255_255", "delta_past_end", "delta_sets_x", "eob_when_full", "no_eol", "trailing_bytes", "handwritten_topdown",
     "handwritten_offset_0", "example_gray", "real_picture"] + [f"picture_{k}" for k in ("rle8", "rle4", "p4", "p1", "rgb565")]
)

# Files Pillow opens that the decoder leaves to it (status 1), by the prefix of the case's name, with the reason.
NAMED_REFUSALS = {
    "rle8_with_4_bits": "the plugin picks the RLE decoder by the compression alone; a crossed depth is nothing a writer produces",
    "rle4_with_8_bits": "the same, the other way round",
    "rle8_with_1_bit": "the same at a depth that has no RLE form at all",
    "p4_gray_identity_palette": "Pillow opens it as mode L and reads the packed bytes as 8-bit samples",
    "p1_gray_identity_palette": "the same at one bit (a palette of one black entry)",
    "p4_black_white_two_colours": "Pillow opens it as mode 1 and reads the 4-bit data as 1-bit",
    "taken_by_ke_bmp": "uncompressed 8-, 24- and 32-bit files are ke_bmp_decode's, which runs first",
}


@functools.lru_cache(maxsize=None)
def invalid_cases():
    """[(name, file, status)]: one rule each.  Status 2: Pillow raises on load.  Status 1: Pillow raises too, or the name starts
    with a key of NAMED_REFUSALS."""
    rng = np.random.default_rng(2028)
    pal8, pal4 = palette(rng, 256), palette(rng, 16)
    s8 = _start(False)
    out = []
    for rle4 in (False, True):
        t = "rle4" if rle4 else "rle8"
        v = (lambda a: (a << 4) | a) if rle4 else (lambda a: a)
        f = lambda w, h, s, **kw: rle_file(w, h, s, rle4=rle4, **kw)
        out.append((f"{t}_early_end_of_bitmap", f(4, 3, run(4, v(1)) + EOL + run(4, v(2)) + EOB), CORRUPT))
        out.append((f"{t}_cut_after_one_byte_of_a_code", f(4, 2, run(4, v(1)) + EOL + b"\x04"), CORRUPT))
        s = Stream(_start(rle4), rle4).add(run(4, v(1)) + EOL).absolute([1, 2, 3, 4, 5, 6, 7, 8]).bytes()
        out.append((f"{t}_cut_inside_an_absolute_payload", f(6, 3, s[:-2]), CORRUPT))
        out.append((f"{t}_cut_inside_a_delta", f(4, 2, run(4, v(1)) + EOL + run(1, v(2)) + b"\x00\x02\x01"), CORRUPT))
        out.append((f"{t}_pixels_short_by_one", f(4, 2, run(4, v(1)) + EOL + run(3, v(2))), CORRUPT))
        out.append((f"{t}_last_row_without_eol_falls_short", f(4, 2, run(4, v(1)) + EOL + run(2, v(2)) + EOB), CORRUPT))
        out.append((f"{t}_no_stream_at_all", f(4, 2, b""), CORRUPT))
        out.append((f"{t}_data_offset_beyond_the_file", f(4, 2, run(4, v(1)) + EOL + run(4, v(2)) + EOB, offset=5000), CORRUPT))
    # rows without padding: the last byte is a pixel's ("image file is truncated"); with padding, see valid_cases
    px4, px1, px16 = _indices(rng, "p4", 8, 4), _indices(rng, "p1", 32, 4), _indices(rng, "rgb555", 2, 4)
    out.append(("p4_pixel_data_short_by_one", picture("p4", px4, pal=pal4)[:-1], CORRUPT))
    out.append(("p1_pixel_data_short_by_one", picture("p1", px1, pal=pal4[:8])[:-1], CORRUPT))
    out.append(("rgb555_pixel_data_short_by_one", picture("rgb555", px16)[:-1], CORRUPT))
    out.append(("rgb565_pixel_data_short_by_one", picture("rgb565", px16)[:-1], CORRUPT))
    out.append(("p4_padded_row_short_by_three", picture("p4", _indices(rng, "p4", 11, 4), pal=pal4)[:-3], CORRUPT))
    px4, px1, px16 = _indices(rng, "p4", 11, 4), _indices(rng, "p1", 11, 4), _indices(rng, "rgb555", 11, 4)
    out.append(("not_a_bmp", b"BA" + picture("p4", px4, pal=pal4)[2:], CORRUPT))
    for k, m in enumerate(((0xF800, 0x7E0, 0x3F), (0x7C00, 0x3E0, 0x1E), (0x1F, 0x7E0, 0xF800), (0, 0, 0), (0xFF0000, 0xFF00, 0xFF))):
        for hs in (40, 124):
            out.append((f"unknown_16_bit_masks_{k}_hs{hs}", Wr.bmp(11, 4, 16, Wr.rows16(px16), hs=hs, comp=3, masks=m), UNSUPPORTED))
    for comp in (4, 5, 6, 255):
        out.append((f"compression_{comp}", Wr.bmp(11, 4, 16, Wr.rows16(px16), comp=comp), UNSUPPORTED))
    stream = run(4, 1) + EOL + run(4, 2) + EOB
    out.append(("rle_with_24_bits", Wr.bmp(4, 2, 24, stream, comp=1), UNSUPPORTED))
    out.append(("rle_with_16_bits", Wr.bmp(4, 2, 16, stream, comp=1), UNSUPPORTED))
    out.append(("rle8_with_1_bit", Wr.bmp(4, 2, 1, stream, comp=1, colors=2, palette=pal4[:8]), UNSUPPORTED))
    out.append(("rle8_with_4_bits", Wr.bmp(4, 2, 4, stream, comp=1, colors=16, palette=pal4), UNSUPPORTED))
    out.append(("rle4_with_8_bits", Wr.bmp(4, 2, 8, stream, comp=2, colors=256, palette=pal8), UNSUPPORTED))
    out.append(("bitfields_with_4_bits", Wr.bmp(11, 4, 4, Wr.rows4(px4), comp=3, masks=M555, colors=16, palette=pal4), UNSUPPORTED))
    # (Pillow opens these up to a width of 4, where a stored row holds a byte per pixel; beyond that it raises)
    out.append(("p4_gray_identity_palette", picture("p4", px4[:, :3], pal=GRAY256[:64]), UNSUPPORTED))
    out.append(("p4_gray_identity_palette_of_3", picture("p4", px4[:, :4], pal=GRAY256[:12]), UNSUPPORTED))
    out.append(("p4_gray_identity_palette_wide", picture("p4", px4, pal=GRAY256[:64]), UNSUPPORTED))
    out.append(("p1_gray_identity_palette_of_1", picture("p1", px1[:, :3], pal=GRAY256[:4]), UNSUPPORTED))
    out.append(("p4_black_white_two_colours", picture("p4", px4 & 1, pal=bytes([0, 0, 0, 0, 255, 255, 255, 0])), UNSUPPORTED))
    out.append(("rle8_black_white_two_colours", rle_file(4, 2, stream, pal=bytes([0, 0, 0, 0, 255, 255, 255, 0])), UNSUPPORTED))
    out.append(("colors_above_256_at_4_bits", picture("p4", px4, pal=palette(rng, 257)), UNSUPPORTED))
    out.append(("rle8_colors_above_256", rle_file(4, 2, stream, pal=palette(rng, 300)), UNSUPPORTED))
    out.append(("palette_leaves_the_file", Wr.bmp(4, 2, 4, b"", colors=16, palette=pal4[:40]), UNSUPPORTED))
    out.append(("bits_2", Wr.bmp(11, 4, 2, bytes(16), colors=4, palette=pal4[:16]), UNSUPPORTED))
    out.append(("os2_header", b"BM" + (26 + 16).to_bytes(4, "little") + bytes(4) + (26).to_bytes(4, "little") + (12).to_bytes(4, "little") +
                bytes([11, 0, 4, 0, 1, 0, 4, 0]) + bytes(16), UNSUPPORTED))
    out.append(("zero_width", Wr.bmp(0, 4, 4, b"", colors=16, palette=pal4), UNSUPPORTED))
    out.append(("taken_by_ke_bmp_8_bits", Wr.bmp(4, 2, 8, bytes(8), colors=256, palette=pal8), UNSUPPORTED))
    out.append(("taken_by_ke_bmp_24_bits", Wr.bmp(4, 2, 24, bytes(24)), UNSUPPORTED))
    assert s8 == 14 + 40 + 1024
    return out


def random_stream(rng, w: int, h: int, rle4: bool, start: int) -> bytes:
    """Codes drawn from every code valid at each point until the pixels they stand for pass W * H -- or, one time in eight, stop
    a little short of it, and one code in 200 is an early end-of-bitmap: Pillow then raises.  The count kept here only decides
    when to stop drawing; what the stream means is Pillow's to say."""
    s = Stream(start, rle4)
    pos = x = 0
    want = w * h if rng.integers(0, 8) else max(0, w * h - int(rng.integers(1, 2 * w + 2)))
    while pos < want:
        c = int(rng.integers(0, 200))
        if c < 90:
            n = int(rng.integers(1, 256)) if rng.integers(0, 6) == 0 else int(rng.integers(1, w + 3))
            n = min(n, 255)
            s.add(run(n, int(rng.integers(0, 256))))
            n = min(n, max(0, w - x))
            pos, x = pos + n, x + n
        elif c < 130:
            s.add(EOL)
            pos, x = pos + (-pos) % w, 0
        elif c < 180:
            n = int(rng.integers(3, 256)) if rng.integers(0, 6) == 0 else int(rng.integers(3, w + 6))
            n = min(n, 255)
            pixels = rng.integers(0, 16 if rle4 else 256, n).tolist()
            if rng.integers(0, 12) == 0:                       # padded by chance, not by the file's parity
                s.add(Wr.absolute(n, bytes(pixels[:n // 2] if rle4 else pixels), pad=bool(rng.integers(0, 2))))
            else:
                s.absolute(pixels)
            pos, x = pos + (n - (n & 1) if rle4 else n), x + n
        elif c < 199:
            r, u = (int(rng.integers(0, 256)), int(rng.integers(0, 256))) if rng.integers(0, 10) == 0 else (int(rng.integers(0, w + 1)), int(rng.integers(0, 2)))
            s.add(delta(r, u))
            pos += r + u * w
            x = pos % w
        else:
            s.add(EOB)
            break
    if rng.integers(0, 4) == 0:
        s.add(EOB)
    return s.bytes()


@functools.lru_cache(maxsize=None)
def random_cases(count: int = 1000):
    """[(name, file)]: random RLE8 / RLE4 code streams for W, H in 1 .. 40, at both parities of the data offset, bottom-up and top-down."""
    rng = np.random.default_rng(2029)
    out = []
    for k in range(count):
        w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        rle4, gap = bool(k & 1), (k >> 1) & 1
        out.append((f"random_{k}", rle_file(w, h, random_stream(rng, w, h, rle4, _start(rle4, gap)), rle4=rle4, gap=gap, topdown=k % 5 == 0)))
    return out


def every_file():
    """[(name, file)] of every set."""
    return [(n, d) for n, d, _ in valid_cases()] + [(n, d) for n, d, _ in invalid_cases()] + list(random_cases())


def fuzz_bases():
    names = ("rle8_13x3", "rle4_13x3", "p1_13x3", "p4_13x3", "rgb555_13x3", "rgb565_13x3", "rle8_absolute_spills_into_next_row", "rle4_delta_up",
             "rle8_picture_drawing_0", "rle4_picture_smooth_1")
    by_name = {n: d for n, d, _ in valid_cases()}
    return [(n, by_name[n]) for n in names]


def byte_changes(count: int = 2000, seed: int = 2030):
    """[(name, file)]: single-byte changes in header, palette and stream of small valid files."""
    rng = np.random.default_rng(seed)
    bases = [(n, d) for n, d in fuzz_bases() if len(d) < 3000]
    out = []
    for k in range(count):
        name, base = bases[k % len(bases)]
        b = bytearray(base)
        region = k % 3
        at = int(rng.integers(2, 54)) if region == 0 else int(rng.integers(54, len(b))) if region == 1 else int(rng.integers(max(54, len(b) - 60), len(b)))
        b[at] = int(rng.integers(0, 256)) if k % 4 else int(rng.choice([0, 1, 2, 3, 4, 8, 16, 40, 255]))
        out.append((f"{name}/byte_{at}", bytes(b)))
    return out
