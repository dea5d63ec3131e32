"""Animated WebP test cases for the decoder of their first frame (kobato-eyes_amd/csrc/ke_webpn_parse.h, ke_webpn.hip): a
container writer that emits exactly the chunks, ANMF header fields and flags it is given, fed with frames taken from the still
case modules (_webp_cases, _webpa_cases, _webpl_cases: their ALPH / "VP8 " / VP8L chunks re-wrapped) and with what Pillow's
``save_all`` writes; the valid families with their census, the invalid cases with the status their rule names, and damage.
Pillow is the reference throughout: ``np.asarray(Image.open(f))`` is frame 0."""
from __future__ import annotations

import functools
import io
import struct
from collections import Counter

import numpy as np
from PIL import Image

import _webp_cases as W
import _webpa_cases as A
import _webpl_cases as L
from _webp_cases import CORRUPT, OK, UNSUPPORTED, chunks, content, exif_blob, riff  # noqa: F401
from _webpa_cases import pillow_pixels  # noqa: F401

ANIMATION, XMP_FLAG, EXIF_FLAG, ALPHA, ICC = 0x02, 0x04, 0x08, 0x10, 0x20
BACKGROUND = 0xC04080FF                                             # a non-zero ANIM background colour: Pillow ignores it
LOSSY, LOSSY_ALPHA, LOSSLESS = "lossy", "lossy_alpha", "lossless"
CODECS = (LOSSY, LOSSY_ALPHA, LOSSLESS)


# ---- the writer -----------------------------------------------------------------------------------------------------------
def chunk(tag: bytes, payload: bytes) -> bytes:
    return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def vp8x(flags: int, canvas: tuple) -> tuple:
    return (b"VP8X", bytes([flags, 0, 0, 0]) + (canvas[0] - 1).to_bytes(3, "little") + (canvas[1] - 1).to_bytes(3, "little"))


def anim(background: int = BACKGROUND, loops: int = 0) -> tuple:
    return (b"ANIM", struct.pack("<IH", background, loops))


def anmf(subs, x: int, y: int, w: int, h: int, duration: int = 100, bits: int = 0) -> tuple:
    """An ANMF chunk: the 16-byte header as given (x and y are stored halved; bits: bit 0 dispose, bit 1 no-blend, the rest
    reserved), then the sub-chunks [(fourcc, payload)]"""
    head = (x // 2).to_bytes(3, "little") + (y // 2).to_bytes(3, "little") + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")
    return (b"ANMF", head + duration.to_bytes(3, "little") + bytes([bits]) + b"".join(chunk(t, p) for t, p in subs))


def animation(canvas: tuple, flags: int, parts) -> bytes:
    """RIFF / WEBP / VP8X (``flags`` as given) / the chunks of ``parts``"""
    return riff([vp8x(flags, canvas), *parts])


class Frame:
    """The sub-chunks of one frame, taken from a still file: [(fourcc, payload)], its size and codec"""

    def __init__(self, still: bytes):
        self.subs = [(t, p) for t, p in chunks(still) if t in (b"ALPH", b"VP8 ", b"VP8L")]
        tags = [t for t, _ in self.subs]
        self.codec = LOSSLESS if b"VP8L" in tags else LOSSY_ALPHA if b"ALPH" in tags else LOSSY
        self.w, self.h = L.image_size(self.subs[0][1]) if self.codec == LOSSLESS else W.frame_size(self.subs[-1][1])

    def at(self, x: int = 0, y: int = 0, **kw) -> tuple:
        return anmf(self.subs, x, y, self.w, self.h, **kw)

    def still(self, alpha_flag: bool) -> bytes:
        """The same sub-chunks as a still file"""
        if self.codec == LOSSLESS:
            return riff(self.subs)
        return riff([vp8x(ALPHA if alpha_flag else 0, (self.w, self.h)), *self.subs])


def simple(frame: Frame, canvas=None, x: int = 0, y: int = 0, alpha: bool = False, more=(), **kw) -> bytes:
    """One frame on a canvas (its own size unless given), further ANMF chunks behind it"""
    return animation(canvas or (frame.w, frame.h), ANIMATION | (ALPHA if alpha else 0), [anim(), frame.at(x, y, **kw), *more])


# ---- frames ---------------------------------------------------------------------------------------------------------------
def _lossy(rng, w, h, kind="smooth", q=70):
    return Frame(W.pillow_file(content(rng, w, h, kind), q, 4))


def _lossy_alpha(rng, w, h, how=0):
    """how: 0..3 a raw plane with that filter, 4..7 a VP8L-coded plane with filter how - 4, 8 what Pillow writes"""
    a = A.plane(rng, w, h, A.ALPHA_KINDS[how % 5])
    if how == 8:
        return Frame(A.pillow_file(content(rng, w, h, "noisy"), a if a.min() < 255 else A.plane(rng, w, h, "noise"), 75, 4, 80))
    if how < 4:
        return Frame(A.mux(A.frame(rng, w, h), A.raw_alph(a, how)))
    g = A.forward_filter(a, how - 4)
    return Frame(A.mux(A.frame(rng, w, h), A.lossless_alph(L.pillow_file(Image.fromarray(np.dstack([g, g, g])), 60, 3), how - 4)))


def _lossless(rng, w, h, rgba=False, kind="drawing"):
    a = content(rng, w, h, kind)
    return Frame(L.pillow_file(L._rgba(rng, a) if rgba else Image.fromarray(a), 70, 3, exact=rgba))


def _frame(rng, codec, w, h, k=0):
    if codec == LOSSY:
        return _lossy(rng, w, h, W.KINDS[k % 5], 40 + 11 * (k % 5))
    if codec == LOSSY_ALPHA:
        return _lossy_alpha(rng, w, h, k % 9)
    return _lossless(rng, w, h, rgba=bool(k % 2), kind=W.KINDS[k % 5])


# ---- the valid families ---------------------------------------------------------------------------------------------------
def pillow_animation(frames, **kw) -> bytes:
    buf = io.BytesIO()
    frames[0].save(buf, "WEBP", save_all=True, append_images=frames[1:], duration=80, **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def valid_cases() -> tuple:
    """((family, name, bytes), ...): every file here is one the decoder has to take and Pillow opens"""
    rng = np.random.default_rng(110)
    out = []
    add = lambda family, name, data: out.append((family, name, data))         # noqa: E731
    # each codec as frame 0 with the VP8X alpha flag on and off, the frame equal to the canvas
    for codec in CODECS:
        for k, (w, h) in enumerate([(38, 22), (16, 16), (33, 47), (64, 40), (5, 3), (100, 9), (17, 31), (48, 48), (70, 21)]):
            f = _frame(rng, codec, w, h, k)
            for alpha in (False, True):
                add("codec_flag", f"{codec}_{k}_{w}x{h}_alpha{int(alpha)}", simple(f, alpha=alpha))
    # still files of the three case modules re-wrapped as they are
    stills = [d for _, d in W.pillow_cases(n=12)] + [d for _, d in W.golden_cases()[:6]] + [d for _, d in A.pillow_cases(n=12)]
    stills += [d for _, d, _ in A.raw_cases()[:12]] + [d for _, d, _ in A.lossless_cases()[:10]] + [d for _, d in L.pillow_cases(n=29)]
    stills += [d for _, d in L.palette_cases()] + [d for _, d in L.golden_cases()[:6]]
    for k, still in enumerate(stills):
        f = Frame(still)
        add("rewrapped", f"{f.codec}_{k}_{f.w}x{f.h}", simple(f, alpha=bool(k % 2)))
    # a 38 x 22 frame at each corner of a larger canvas, and centred
    for codec in CODECS:
        f = _frame(rng, codec, 38, 22, 3)
        for alpha in (False, True):
            for name, (x, y) in {"nw": (0, 0), "ne": (12, 0), "sw": (0, 12), "se": (12, 12), "centre": (6, 6)}.items():
                add("placed", f"{codec}_{name}_alpha{int(alpha)}", simple(f, (50, 34), x, y, alpha))
        add("placed", f"{codec}_issue_48x32_at_4_6", simple(f, (48, 32), 4, 6, True))
    # the smallest canvases and frames
    for k, codec in enumerate(CODECS):
        dot, tall, flat = _frame(rng, codec, 1, 1, k), _frame(rng, codec, 1, 17, k), _frame(rng, codec, 17, 1, k)
        for alpha in (False, True):
            add("tiny", f"{codec}_1x1_on_1x1_alpha{int(alpha)}", simple(dot, alpha=alpha))
            add("tiny", f"{codec}_1x1_at_2_2_of_3x3_alpha{int(alpha)}", simple(dot, (3, 3), 2, 2, alpha))
            add("tiny", f"{codec}_1_wide_alpha{int(alpha)}", simple(tall, (7, 21), 4, 2, alpha))
            add("tiny", f"{codec}_1_high_alpha{int(alpha)}", simple(flat, (23, 5), 6, 4, alpha))
    # canvas widths 1..9 and 15..17 with 3 and 4 channels: the store-alignment paths
    for k, cw in enumerate(list(range(1, 10)) + [15, 16, 17]):
        for alpha in (False, True):
            f = _frame(rng, CODECS[(k + alpha) % 3], cw, 3 + k % 3, k)
            add("widths", f"w{cw}_alpha{int(alpha)}_{f.codec}_whole", simple(f, alpha=alpha))
            if cw >= 3:
                g = _frame(rng, CODECS[(k + alpha + 1) % 3], cw - 2, 2, k)
                add("widths", f"w{cw}_alpha{int(alpha)}_{g.codec}_inset", simple(g, (cw, 5), 2, 2, alpha))
    # one frame, two frames, many frames; later frames of another codec; a later frame that is garbage behind its header
    for k, codec in enumerate(CODECS):
        first = _frame(rng, codec, 30, 20, k)
        others = [_frame(rng, CODECS[(k + 1 + j) % 3], 12 + 2 * j, 10, j) for j in range(11)]
        add("frames", f"{codec}_1_frame", simple(first, (40, 30), 2, 2))
        add("frames", f"{codec}_2_frames_other_codec", simple(first, (40, 30), 2, 2, True, [others[0].at(4, 6)]))
        add("frames", f"{codec}_12_frames", simple(first, (40, 30), 2, 2, False, [o.at(2 * (j % 4), 4, bits=j % 4) for j, o in enumerate(others)]))
        for o in others[:2]:
            tail = o.subs[-1]
            head = 10 if tail[0] == b"VP8 " else 5
            junk = tail[1][:head] + rng.integers(0, 256, len(tail[1]) - head, dtype=np.uint8).tobytes()
            add("frames", f"{codec}_later_{o.codec}_garbage", simple(first, (40, 30), 2, 2, True, [anmf(o.subs[:-1] + [(tail[0], junk)], 0, 0, o.w, o.h)]))
    # every blend and dispose bit on frame 0, another background, loop counts
    for k, codec in enumerate(CODECS):
        f = _frame(rng, codec, 20, 14, k + 1)
        for bits in range(4):
            add("bits", f"{codec}_bits{bits}", simple(f, (24, 18), 2, 4, bool(bits & 1), bits=bits, duration=bits * 1000))
        add("background", f"{codec}_background", animation((24, 18), ANIMATION | ALPHA, [anim(0xFFFFFFFF, 3), f.at(4, 2)]))
        add("background", f"{codec}_background_0", animation((24, 18), ANIMATION, [anim(0, 65535), f.at(4, 2)]))
    # unknown chunks between frames and inside ANMF (behind the image), ICCP, EXIF / XMP chunks
    for k, codec in enumerate(CODECS):
        f, g = _frame(rng, codec, 26, 18, k + 2), _frame(rng, CODECS[(k + 1) % 3], 10, 10, k)
        inside = anmf(f.subs + [(b"ZZZZ", b"12345")], 2, 2, f.w, f.h)
        add("unknown", f"{codec}_between", animation((30, 22), ANIMATION, [anim(), (b"JUNK", b"abc"), f.at(2, 2), (b"ZZZZ", b"1234"), g.at(), (b"TAIL", b"")]))
        add("unknown", f"{codec}_inside", animation((30, 22), ANIMATION | ALPHA, [anim(), inside, g.at()]))
        add("unknown", f"{codec}_second_anim", animation((30, 22), ANIMATION, [anim(), f.at(2, 2), anim(1, 1), g.at()]))
        add("meta", f"{codec}_iccp", animation((30, 22), ANIMATION | ICC, [(b"ICCP", b"\0" * 131), anim(), f.at(2, 2)]))
        add("meta", f"{codec}_exif", animation((30, 22), ANIMATION | EXIF_FLAG | ALPHA, [anim(), f.at(2, 2), (b"EXIF", exif_blob())]))
        add("meta", f"{codec}_xmp", animation((30, 22), ANIMATION | XMP_FLAG, [anim(), f.at(2, 2), g.at(), (b"XMP ", W.XMP_TURNED)]))
    # what Pillow's save_all writes
    for k in range(12):
        w, h = [(32, 32), (57, 41), (9, 13), (120, 64)][k % 4]
        n = (2, 3, 5)[k % 3]
        pics = [content(rng, w, h, W.KINDS[(k + j) % 5]) for j in range(n)]
        if k % 4 >= 2:
            pics = [np.dstack([p, A.plane(rng, w, h, A.ALPHA_KINDS[(k + j) % 5])]) for j, p in enumerate(pics)]
        kw = dict(lossless=True) if k % 3 == 1 else dict(quality=30 + 5 * k, allow_mixed=k % 3 == 2, minimize_size=k % 2 == 1)
        add("pillow", f"save_all_{k}_{w}x{h}_{n}_frames", pillow_animation([Image.fromarray(p) for p in pics], **kw))
    return tuple(out)


FAMILIES = ("codec_flag", "rewrapped", "placed", "tiny", "widths", "frames", "bits", "background", "unknown", "meta", "pillow")


def census() -> Counter:
    """Files per family, per frame-0 codec and per channel count"""
    count = Counter()
    for family, name, data in valid_cases():
        count[family] += 1
        first = next(p for t, p in chunks(data) if t == b"ANMF")
        tags = [t for t, _ in chunks(b"\0" * 12 + first[16:])]
        count[LOSSLESS if tags[0] == b"VP8L" else LOSSY_ALPHA if tags[0] == b"ALPH" else LOSSY] += 1
        count["rgba" if data[20] & ALPHA else "rgb"] += 1
    return count


def with_meta(data: bytes) -> bool:
    return any(t in (b"EXIF", b"XMP ") for t, _ in chunks(data))


# ---- the invalid cases ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def invalid_cases() -> tuple:
    """((name, bytes, expected status), ...): each breaks one rule of the demuxer's; CORRUPT is what Pillow fails on"""
    rng = np.random.default_rng(111)
    f, g, a = _lossy(rng, 38, 22), _lossless(rng, 20, 12), _lossy_alpha(rng, 38, 22, 1)
    good = simple(f, (48, 32), 4, 6, True, [g.at(2, 2)])
    out = [("flag_without_anmf", animation((38, 22), ANIMATION, [anim()]), CORRUPT),
           ("flag_with_a_bare_frame", animation((38, 22), ANIMATION, [anim(), *f.subs]), CORRUPT),
           ("reserved_flag_bit", animation((48, 32), ANIMATION | 0x01, [anim(), f.at(4, 6)]), CORRUPT),
           ("frame_right_of_canvas", simple(f, (48, 32), 12, 6), CORRUPT),
           ("frame_below_canvas", simple(f, (48, 32), 4, 12), CORRUPT),
           ("later_frame_outside_canvas", simple(f, (48, 32), 4, 6, False, [g.at(30, 2)]), CORRUPT),
           ("alph_behind_vp8", animation((48, 32), ANIMATION | ALPHA, [anim(), anmf(a.subs[::-1], 4, 6, a.w, a.h)]), CORRUPT),
           ("alph_before_vp8l", animation((48, 32), ANIMATION | ALPHA, [anim(), anmf([a.subs[0], *g.subs], 4, 6, g.w, g.h)]), CORRUPT),
           ("anim_missing", animation((48, 32), ANIMATION, [f.at(4, 6)]), CORRUPT),
           ("anim_behind_anmf", animation((48, 32), ANIMATION, [f.at(4, 6), anim()]), CORRUPT),
           ("anim_too_short", animation((48, 32), ANIMATION, [(b"ANIM", b"\0\0\0\0"), f.at(4, 6)]), CORRUPT),
           ("anmf_header_short", animation((48, 32), ANIMATION, [anim(), f.at(4, 6), (b"ANMF", b"\0" * 12)]), CORRUPT),
           ("second_vp8x", animation((48, 32), ANIMATION, [anim(), f.at(4, 6), vp8x(ANIMATION, (48, 32))]), CORRUPT),
           ("alph_alone", animation((48, 32), ANIMATION | ALPHA, [anim(), anmf(a.subs[:1], 4, 6, a.w, a.h)]), CORRUPT),
           ("cut_in_frame_0", good[: good.find(b"VP8 ") + 40], CORRUPT),
           ("cut_in_a_later_frame", good[: good.find(b"VP8L") + 20], CORRUPT),
           ("cut_last_byte", good[:-1], CORRUPT)]
    short = bytearray(good)                                         # the RIFF size ends inside the later frame
    short[4:8] = struct.pack("<I", good.find(b"VP8L") + 20 - 8)
    out.append(("riff_size_cut_in_a_later_frame", bytes(short), CORRUPT))
    long = bytearray(good)
    long[4:8] = struct.pack("<I", len(good) + 100)
    out.append(("riff_too_long", bytes(long), CORRUPT))
    inter = bytearray(f.subs[0][1])
    inter[0] |= 1
    out.append(("later_inter_frame", simple(g, (48, 32), 0, 0, False, [anmf([(b"VP8 ", bytes(inter))], 4, 6, f.w, f.h)]), CORRUPT))
    sig = bytearray(g.subs[0][1])
    sig[0] = 0x2E
    out.append(("later_vp8l_signature", simple(f, (48, 32), 4, 6, False, [anmf([(b"VP8L", bytes(sig))], 0, 0, g.w, g.h)]), CORRUPT))
    # left to Pillow: without the flag a file is a still decoder's, whatever else it holds; an ANMF chunk without an image at its front is left alone (Pillow fails these)
    out.append(("anmf_without_flag", animation((48, 32), 0, [anim(), f.at(4, 6)]), UNSUPPORTED))
    out.append(("anmf_without_flag_alpha", animation((48, 32), ALPHA, [anim(), a.at(4, 6)]), UNSUPPORTED))
    out.append(("still_lossy", W.pillow_file(content(rng, 38, 22, "smooth"), 70, 4), UNSUPPORTED))
    out.append(("still_vp8x", f.still(False), UNSUPPORTED))
    out.append(("still_alpha", a.still(True), UNSUPPORTED))
    out.append(("still_lossless", g.still(False), UNSUPPORTED))
    out.append(("unknown_in_front_of_the_image", animation((48, 32), ANIMATION, [anim(), anmf([(b"ZZZZ", b"12"), *f.subs], 4, 6, f.w, f.h)]), UNSUPPORTED))
    out.append(("vp8x_of_12_bytes", riff([(b"VP8X", vp8x(ANIMATION, (48, 32))[1] + b"\0\0"), anim(), f.at(4, 6)]), UNSUPPORTED))
    out.append(("not_webp", b"RIFF" + struct.pack("<I", 100) + b"WAVE" + b"\0" * 96, UNSUPPORTED))
    out.append(("empty", b"", UNSUPPORTED))
    return tuple(out)


# Refusals Pillow does not share: files the decoder leaves to Pillow (status 1) although Pillow opens them, each with its reason.
UNSHARED_REFUSALS = {
    "anmf_wider_than_bitstream": "an ANMF header whose size is not its bitstream's: libwebp 1.6 takes the bitstream's size and "
                                 "Pillow shows the frame; refused, the header being what places the frame here",
    "anmf_shorter_than_bitstream": "as above",
    "later_anmf_size_differs": "as above, in a later frame",
    "empty_anmf": "an ANMF chunk with no image in it is no frame to the demuxer: refused, since which frame is frame 0 then "
                  "depends on it",
    "canvas_over_cap": "a canvas over 2^24 pixels: the cap the lossless decoder puts on an image",
    "frame_0_over_the_lossy_cap": "does not occur: a lossy frame over 65 536 macroblocks needs a canvas over the cap above",
}


@functools.lru_cache(maxsize=None)
def unshared_cases() -> tuple:
    """((name, bytes), ...) of UNSHARED_REFUSALS, where a file can be written"""
    rng = np.random.default_rng(112)
    f = _lossy(rng, 38, 22)
    g = _lossless(rng, 20, 12)
    out = [("anmf_wider_than_bitstream", animation((48, 32), ANIMATION, [anim(), anmf(f.subs, 4, 6, f.w + 1, f.h)])),
           ("anmf_shorter_than_bitstream", animation((48, 32), ANIMATION, [anim(), anmf(f.subs, 4, 6, f.w, f.h - 1)])),
           ("later_anmf_size_differs", simple(f, (48, 32), 4, 6, False, [anmf(g.subs, 0, 0, g.w + 2, g.h)])),
           ("empty_anmf", animation((48, 32), ANIMATION, [anim(), f.at(4, 6), (b"ANMF", b"\0" * 16), f.at(2, 2)])),
           ("canvas_over_cap", simple(f, (4097, 4097), 4, 6))]
    return tuple(out)


# ---- damage ---------------------------------------------------------------------------------------------------------------
CUTS = ("half", "last_byte", "byte_30")


def cut_cases() -> list:
    """Every valid file cut at half its length, before its last byte and at byte 30 (inside the ANIM chunk): [(name, bytes)]"""
    out = []
    for _, name, data in valid_cases():
        out += [(f"{name}_cut_half", data[: len(data) // 2]), (f"{name}_cut_last_byte", data[:-1]), (f"{name}_cut_byte_30", data[:30])]
    return out


def byte_changes(count: int = 2000, seed: int = 113) -> list:
    """``count`` files, each a valid one with a single byte behind the RIFF header replaced by another value: [(name, bytes)]"""
    rng = np.random.default_rng(seed)
    cases = valid_cases()
    out = []
    for k in range(count):
        _, name, data = cases[k % len(cases)]
        b = bytearray(data)
        at = int(rng.integers(12, len(b)))
        b[at] = (b[at] + int(rng.integers(1, 256))) & 255
        out.append((f"{name}_byte_{at}", bytes(b)))
    return out
