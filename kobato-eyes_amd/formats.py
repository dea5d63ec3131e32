"""The formats the GPU decoders take: one row per ``ke_<kind>_{probe,decode,caveats}`` triple of include/keyes.h, and which of
them a seam offers its files to under the current environment.  The binding (_native), the batch hasher (fastsig) and the two
refine routes (refine, refine_parallel) all read this table; adding a decoder adds a row."""
from __future__ import annotations

import os
from typing import NamedTuple, Optional


class Format(NamedTuple):
    kind: str                  # the <kind> of ke_<kind>_probe / _decode / _caveats and of Context.probe / decode / hash
    suffixes: tuple            # lower-case file suffixes whose files are offered to the decoder
    off_switch: str            # <variable>=0 turns the decoder off, and the decoders that follow it
    opt_in: Optional[str]      # <variable>=1 turns the decoder on (None: on unless switched off)
    follows: Optional[str]     # the kind whose UNSUPPORTED (status 1) files this decoder is offered, after that one has run
    luma_only: bool            # the decoder yields the luma the hashes see, not the picture: only the hashing seams take it
    decodes: str               # Context.<kind>_decode's docstring


_TIFF_SHAPES = "HxW gray or luma of a palette file, HxWx3, HxWx4"
FORMATS = (
    Format("jpeg", (".jpg", ".jpeg", ".jpe", ".jfif"), "KE_GPU_JPEG", None, None, False,
           "Pixels of JPEG files decoded on the GPU (HxW or HxWx3, what np.asarray(Image.open(f)) gives)"),
    Format("png", (".png", ".apng"), "KE_GPU_PNG", None, None, False,
           "Pixels of PNG files decoded on the GPU (HxW, HxWx3 or HxWx4)"),
    Format("bmp", (".bmp",), "KE_GPU_BMP", None, None, False,
           "Pixels of uncompressed BMP files unpacked on the GPU (HxW luma of a palette file, HxWx3 or HxWx4)"),
    Format("bmpx", (".bmp",), "KE_GPU_BMP", "KE_GPU_BMP_EXTENDED", "bmp", False,
           "Pixels of RLE8 / RLE4, uncompressed 1- and 4-bit and 16-bit BMP files decoded on the GPU (HxW luma of a palette file, HxWx3 "
           "of a 16-bit file)"),
    Format("gif", (".gif",), "KE_GPU_GIF", None, None, True,
           'Luma (HxW) of the first frame of GIF files decoded on the GPU -- what ``Image.open(f).convert("L")`` yields'),
    Format("tiff", (".tif", ".tiff"), "KE_GPU_TIFF", None, None, False,
           f"Pixels of uncompressed 8-bit TIFF files unpacked on the GPU ({_TIFF_SHAPES})"),
    Format("tiffc", (".tif", ".tiff"), "KE_GPU_TIFF", "KE_GPU_TIFF_COMPRESSED", "tiff", False,
           "Pixels of LZW and PackBits 8-bit TIFF files decoded on the GPU (the shapes of ``tiff_decode``)"),
    Format("tiffz", (".tif", ".tiff"), "KE_GPU_TIFF", "KE_GPU_TIFF_DEFLATE", "tiff", False,
           "Pixels of deflate-compressed 8-bit TIFF files (Compression 8 or 32946) decoded on the GPU (the shapes of ``tiff_decode``)"),
    Format("webp", (".webp",), "KE_GPU_WEBP", None, None, False,
           'RGB pixels (HxWx3) of lossy WebP files decoded on the GPU -- what ``Image.open(f).convert("RGB")`` yields'),
    Format("webpl", (".webp",), "KE_GPU_WEBP", "KE_GPU_WEBP_LOSSLESS", "webp", False,
           "Pixels of lossless WebP files (one VP8L bitstream) decoded on the GPU, as ``Image.open(f)`` yields them -- HxWx3 RGB, "
           "or HxWx4 RGBA where Pillow opens the file as RGBA"),
    Format("webpa", (".webp",), "KE_GPU_WEBP", "KE_GPU_WEBP_ALPHA", "webp", False,
           "RGBA pixels (HxWx4) of lossy WebP files with an alpha plane (one VP8 key frame + an ALPH chunk, or the VP8X alpha "
           "flag alone) decoded on the GPU, as ``Image.open(f)`` yields them"),
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
    the luma-only decoders; "refine_parallel" runs every suffix's own decoder before any follow-up."""
    if seam not in ("hash", "refine", "refine_parallel"):
        raise ValueError(f"unknown seam {seam!r}")
    if seam != "hash" and os.environ.get("KE_GPU_REFINE_DECODE", "1") == "0":
        return []
    rows = [f for f in FORMATS
            if os.environ.get(f.off_switch, "1") != "0" and (f.opt_in is None or os.environ.get(f.opt_in, "0") == "1")
            and not (seam == "refine" and f.luma_only)]
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
