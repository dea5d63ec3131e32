"""The formats the GPU decoders take: one row per ``ke_<kind>_{probe,decode,caveats}`` triple of include/keyes.h, which of them a
seam offers its files to under the current environment (``enabled_kinds``, ``Offers``), and what a refine seam does with a file
a decoder hands back (``seam_actions``).  The binding (_native), the batch hasher (fastsig) and the two refine routes (refine,
refine_parallel) all read this table; adding a decoder adds a row."""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import numpy as np

# the bits of ke_<kind>_caveats (KE_CAVEAT_* of include/keyes.h): what the reference's loader would do to the file beyond Image.open
CAVEAT_ORIENTATION = 1         # an EXIF orientation to apply, or a chunk that may hold one
CAVEAT_TRANSPARENCY = 2        # alpha to composite over white
_CAVEATS = CAVEAT_ORIENTATION | CAVEAT_TRANSPARENCY
ORIENTATION_SHIFT = 8          # bits 8..11: the orientation itself (1..8), from the decoders whose row says ``orientation_number``


class Format(NamedTuple):
    kind: str                  # the <kind> of ke_<kind>_probe / _decode / _caveats and of Context.probe / decode / hash
    suffixes: tuple            # lower-case file suffixes whose files are offered to the decoder
    off_switch: str            # <variable>=0 turns the decoder off, and the decoders that follow it
    opt_in: Optional[str]      # <variable>=1 turns the decoder on (None: on unless switched off)
    follows: Optional[str]     # the kind whose UNSUPPORTED (status 1) files this decoder is offered, after that one has run
    luma_only: bool            # the decoder yields the luma the hashes see, not the picture: only the hashing seams take it
    decodes: str               # Context.<kind>_decode's docstring
    # what the refine seams do with the decoder's files (seam_actions)
    orientation_number: bool = False            # the caveats carry the orientation itself: the seams can turn the file on the device
    rgba_leave: Optional[int] = None            # refine: the flag bits that send an RGBA file to the loader, not over white on the device (None: always)
    luma_leave: int = CAVEAT_ORIENTATION        # refine_parallel: the flag bits that keep a file from being used as decoded
    hash_only: bool = False                     # only the hashing seam offers the decoder its files; at the refine seams they go to the loader


_TIFF_SHAPES = "HxW gray or luma of a palette file, HxWx3, HxWx4"
FORMATS = (
    Format("jpeg", (".jpg", ".jpeg", ".jpe", ".jfif"), "KE_GPU_JPEG", None, None, False,
           "Pixels of JPEG files decoded on the GPU (HxW or HxWx3, what np.asarray(Image.open(f)) gives)", orientation_number=True),
    Format("png", (".png", ".apng"), "KE_GPU_PNG", None, None, False,
           "Pixels of PNG files decoded on the GPU (HxW, HxWx3 or HxWx4)", rgba_leave=_CAVEATS),
    Format("bmp", (".bmp",), "KE_GPU_BMP", None, None, False,
           "Pixels of uncompressed BMP files unpacked on the GPU (HxW luma of a palette file, HxWx3 or HxWx4)", rgba_leave=_CAVEATS),
    Format("bmpx", (".bmp",), "KE_GPU_BMP", "KE_GPU_BMP_EXTENDED", "bmp", False,
           "Pixels of RLE8 / RLE4, uncompressed 1- and 4-bit and 16-bit BMP files decoded on the GPU (HxW luma of a palette file, HxWx3 "
           "of a 16-bit file)"),
    Format("gif", (".gif",), "KE_GPU_GIF", None, None, True,
           'Luma (HxW) of the first frame of GIF files decoded on the GPU -- what ``Image.open(f).convert("L")`` yields'),
    Format("tiff", (".tif", ".tiff"), "KE_GPU_TIFF", None, None, False,
           f"Pixels of uncompressed 8-bit TIFF files unpacked on the GPU ({_TIFF_SHAPES})", rgba_leave=_CAVEATS),
    Format("tiffc", (".tif", ".tiff"), "KE_GPU_TIFF", "KE_GPU_TIFF_COMPRESSED", "tiff", False,
           "Pixels of LZW and PackBits 8-bit TIFF files decoded on the GPU (the shapes of ``tiff_decode``)", rgba_leave=_CAVEATS),
    Format("tiffz", (".tif", ".tiff"), "KE_GPU_TIFF", "KE_GPU_TIFF_DEFLATE", "tiff", False,
           "Pixels of deflate-compressed 8-bit TIFF files (Compression 8 or 32946) decoded on the GPU (the shapes of ``tiff_decode``)",
           rgba_leave=_CAVEATS),
    Format("webp", (".webp",), "KE_GPU_WEBP", None, None, False,
           'RGB pixels (HxWx3) of lossy WebP files decoded on the GPU -- what ``Image.open(f).convert("RGB")`` yields'),
    Format("webpl", (".webp",), "KE_GPU_WEBP", "KE_GPU_WEBP_LOSSLESS", "webp", False,
           "Pixels of lossless WebP files (one VP8L bitstream) decoded on the GPU, as ``Image.open(f)`` yields them -- HxWx3 RGB, "
           "or HxWx4 RGBA where Pillow opens the file as RGBA", luma_leave=_CAVEATS),    # an RGBA file stays with the loader
    Format("webpa", (".webp",), "KE_GPU_WEBP", "KE_GPU_WEBP_ALPHA", "webp", False,
           "RGBA pixels (HxWx4) of lossy WebP files with an alpha plane (one VP8 key frame + an ALPH chunk, or the VP8X alpha "
           "flag alone) decoded on the GPU, as ``Image.open(f)`` yields them",
           rgba_leave=CAVEAT_ORIENTATION),       # every file it takes carries the transparency bit: the orientation decides
    Format("webpn", (".webp",), "KE_GPU_WEBP", "KE_GPU_WEBP_ANIMATED", "webp", False,
           "Frame 0 of animated WebP files decoded on the GPU, as ``Image.open(f)`` yields it -- the zeroed canvas with the frame in "
           "its rectangle, HxWx4 RGBA where the VP8X alpha flag is set, HxWx3 RGB otherwise", hash_only=True),
)
KINDS = tuple(f.kind for f in FORMATS)
# the kinds a file's suffix alone assigns it to -- the order in which a hashing batch's files lie in the read-ahead buffer
BASE_KINDS = tuple(f.kind for f in FORMATS if f.follows is None)


def follow_ups(kind: str) -> tuple:
    """The kinds offered what ``kind``'s decoder left UNSUPPORTED, in the order they are tried."""
    return tuple(f.kind for f in FORMATS if f.follows == kind)


def enabled_kinds(seam: str) -> list:
    """[(kind, suffixes)] of the decoders a seam offers its files to, in the order it tries them, under the current environment.

    ``seam``: "hash" (fastsig's batch hasher), "refine" (refine.refine_pairs) or "refine_parallel" (the thumbnail route).  A
    decoder is on unless its off-switch is "0" -- which also takes the decoders that follow it --, an opt-in decoder only when
    its variable is "1".  ``KE_GPU_REFINE_DECODE=0`` turns both refine routes off; "refine" compares pictures and leaves out
    the luma-only decoders; "refine_parallel" runs every suffix's own decoder before any follow-up; neither refine route offers
    a ``hash_only`` decoder anything."""
    if seam not in ("hash", "refine", "refine_parallel"):
        raise ValueError(f"unknown seam {seam!r}")
    if seam != "hash" and os.environ.get("KE_GPU_REFINE_DECODE", "1") == "0":
        return []
    rows = [f for f in FORMATS
            if os.environ.get(f.off_switch, "1") != "0" and (f.opt_in is None or os.environ.get(f.opt_in, "0") == "1")
            and not (seam == "refine" and f.luma_only) and not (seam != "hash" and f.hash_only)]
    if seam == "refine_parallel":
        rows.sort(key=lambda f: f.follows is not None)
    return [(f.kind, f.suffixes) for f in rows]


def files_offered(kind: str, candidates, ran: dict) -> list:
    """``Format.follows`` at the two refine seams: of ``candidates``, the files the seam offers ``kind``'s decoder.  A base kind
    is offered them all; a follow-up only those its base returned UNSUPPORTED (status 1) in this run -- ``ran``: {kind: (paths,
    status)} of the decoders that have run --, nothing if its base did not run.  (No follow-up decoder takes a file its base
    gives another status: tests/test_host_logic.py holds the probes to that.)"""
    base = next(f.follows for f in FORMATS if f.kind == kind)
    if base is None:
        return list(candidates)
    left = {p for p, s in zip(*ran.get(base, ((), ()))) if s == 1}
    return [p for p in candidates if p in left]


class Offers:
    """A refine seam's files on their way through the decoders: iterating yields (kind, the files that kind is offered) for
    every enabled kind of the seam that is offered any, in order -- the files of its suffixes (``paths``: str or Path) that are
    not yet in ``placed`` (the caller's mapping of the files it has dealt with), a follow-up only those its base left.  The
    seam reports every decode call that returned with ``ran``; a call it does not report offers its files to no follow-up."""

    def __init__(self, seam: str, paths, placed):
        self.kinds = enabled_kinds(seam)
        self._paths, self._placed, self._ran = paths, placed, {}

    def __iter__(self):
        for kind, suffixes in self.kinds:
            mine = files_offered(kind, [p for p in self._paths if str(p).lower().endswith(suffixes) and p not in self._placed], self._ran)
            if mine:
                yield kind, mine

    def ran(self, kind: str, paths, status) -> None:
        done = self._ran.setdefault(kind, ([], []))
        done[0].extend(paths)
        done[1].extend(status.tolist())


def decoded_bytes_estimate(path) -> int:
    """Rough decoded size of a compressed file (0 for one that cannot be asked); only paces the seams' runs."""
    try:
        return 48 * os.path.getsize(path)
    except OSError:
        return 0


LEAVE, AS_DECODED, NORMALISE, SHRINK, TURN_SHRINK, SHRINK_OVERSIZE = range(6)    # seam_actions' answers
TURN = NORMALISE                                                     # at the luma seam, where there is no alpha to composite
# what SHRINK_OVERSIZE takes: a decoded image (for a JPEG file: as drafted) of at most this many pixels.  It is the JPEG
# parser's own limit; the route holds the image, its turned copy and the reduced one or the three planes at once, at most
# 9 bytes a pixel (2.4 GB at the bound).
OVERSIZE_MAX_PIXELS = 1 << 28
# ... with a longer side of at most this many times ``max_side``: ke_reduce_rgb's factors end at 255.  The longer side's factor
# is int(longer / max_side / 2); the shorter side's target is its share of max_side brought to a whole number of at least 1,
# which is never below two thirds of that share, so its factor does not pass 1.5 * longer / max_side / 2 = 192 here.
OVERSIZE_MAX_RATIO = 256
# ... and only for a ``max_side`` up to this: the resampler behind ke_thumbnail_rgb_box writes at most 4096 samples per side.
OVERSIZE_MAX_SIDE = 4096


def oversize_enabled() -> bool:
    """``KE_GPU_REFINE_OVERSIZE=1``: the refine seam shrinks files of any size on the device (SHRINK_OVERSIZE)."""
    return os.environ.get("KE_GPU_REFINE_OVERSIZE", "0") == "1"


def seam_actions(kind: str, seam: str, w, h, c, st, flags, max_side: Optional[int] = None, *, oversize: bool = False):
    """What a refine seam does with each file of one decode call of ``kind`` (the arrays decode_files_owned returned): (actions,
    orientations) -- the orientation to apply where the action turns the file, 1 elsewhere.

    "refine" hands pictures over as the reference's loader does (src/utils/image_io.py:107-138): AS_DECODED where all of that
    is a no-op (RGB, no flag, no side over ``max_side``), NORMALISE where the orientation is applied or RGBA composited over
    white on the device, SHRINK / TURN_SHRINK for a longer side, LEAVE to the loader otherwise.  "refine_parallel" shrinks
    what Image.open + exif_transpose yields (src/ui/dup_refine_parallel.py:67-70): AS_DECODED, TURN first, or LEAVE."""
    row = next(f for f in FORMATS if f.kind == kind)
    taken, orient = st == 0, (flags >> ORIENTATION_SHIFT) & 15
    turn = (c == 3) & (orient >= 2) & (orient <= 8) if row.orientation_number else np.zeros(len(st), bool)
    if seam == "refine_parallel":
        turn &= (flags & CAVEAT_ORIENTATION) != 0
        actions = np.select([taken & ((flags & row.luma_leave) == 0), taken & turn], [AS_DECODED, TURN], LEAVE)
        return actions, np.where(turn, orient, 1)
    plain = (c == 3) & ((flags & _CAVEATS) == 0)
    turn &= (flags & _CAVEATS) == CAVEAT_ORIENTATION
    over = (c == 4) & ((flags & row.rgba_leave) == 0) if row.rgba_leave is not None else np.zeros(len(st), bool)
    # a side over max_side: the loader's img.thumbnail((max_side, max_side), LANCZOS) (src/utils/image_io.py:122-124), after the
    # turn.  Below twice that size neither JPEG draft mode nor thumbnail's reducing_gap changes what is resampled (both act
    # from a factor of two on); larger files and those with an alpha channel stay with the loader.
    longest = np.maximum(w, h)
    fits, big = taken & (longest <= max_side), taken & (longest > max_side) & (longest < 2 * max_side - 256)
    actions = np.select([fits & plain, fits & (turn | over), big & plain, big & turn], [AS_DECODED, NORMALISE, SHRINK, TURN_SHRINK], LEAVE)
    if oversize:
        # past that window: SHRINK_OVERSIZE does what thumbnail's reducing_gap adds (Image.reduce, then the resample through a
        # fractional box), after the turn where ``orientations`` says so; the JPEG seam has decoded the file as drafted, so
        # (w, h) are the drafted sizes.  RGBA files (Pillow resamples them premultiplied), gray files and images of more than
        # OVERSIZE_MAX_PIXELS, or longer than OVERSIZE_MAX_RATIO times max_side, stay with the loader, and so does every file
        # when max_side is over OVERSIZE_MAX_SIDE: what the kernels behind the action refuse is not sent to them.
        # Below max_side = 256 the window above is empty (`2 * max_side - 256` is under max_side): the action then starts right
        # behind the `fits` cells, which it never overrides -- the loader shrinks nothing that fits.
        huge = taken & (longest > max_side) & (longest >= 2 * max_side - 256) & (w.astype(np.int64) * h <= OVERSIZE_MAX_PIXELS)
        huge &= (longest.astype(np.int64) <= OVERSIZE_MAX_RATIO * max_side) & (max_side <= OVERSIZE_MAX_SIDE)
        actions = np.where(huge & (plain | turn), SHRINK_OVERSIZE, actions)
    return actions, np.where(turn, orient, 1)
